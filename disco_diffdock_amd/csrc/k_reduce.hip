// The two fixed-order reductions of the training ops (ddk_internal.h): the slice reduction that ends every parameter pass (k_rtp.hip, k_rhid.hip, k_hconv.hip,
// k_eemb.hip) and the segmented sum / mean over a node's edges (the radial conv, the radial hidden layer, the head convs, ddk_seg_sum).  Plain loads, separate
// adds in a written-out order and plain stores, no atomics (compiled with -ffp-contract=off): the bits of a parameter gradient and of a node row depend on
// the operands alone, not on the run, the device or the subset of outputs asked for.  Both are bound by their reads; shapes are run-time values.
#include "ddk_internal.h"

namespace ddk {

struct ReduceArgs { const float* img; ReducePart p0, p1; int n_groups, first[4], count[4]; };      // a group's first slice and its slice count: made on the host

// one thread per element of a group's image: the group's slice images added in slice order, then sent to the weight or the bias gradient of its part
__global__ __launch_bounds__(256) void slice_reduce_kernel(ReduceArgs a) {
  const int idx = blockIdx.x * 256 + threadIdx.x;      // (fewer than 2^20 elements)
  const int n0 = a.p0.rows * (a.p0.cols + 1), PER = n0 + a.p1.rows * (a.p1.cols + 1);
  if (idx >= PER * a.n_groups) return;
  const int grp = idx / PER, rem = idx - grp * PER;
  int first = 0, ns = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (q == grp) { first = a.first[q]; ns = a.count[q]; }
  float sum = 0.f;
  for (int s = 0; s < ns; ++s) sum += a.img[(int64_t)(first + s) * PER + rem];
  const bool second = rem >= n0;
  const ReducePart p = second ? a.p1 : a.p0;
  const int r = second ? rem - n0 : rem, row = r / (p.cols + 1), col = r - row * (p.cols + 1);
  if (col < p.cols) {
    if (p.w) p.w[((int64_t)grp * p.rows + row) * p.cols + col] = sum;
  } else if (p.b) {
    p.b[(int64_t)grp * p.rows + row] = sum;
  }
}

hipError_t launch_slice_reduce(const float* images, const EdgeGroupTable& t, int64_t L, const ReducePart& p0, const ReducePart& p1, hipStream_t s) {
  ReduceArgs a{images, p0, p1, t.n_groups, {}, {}};
  for (int q = 0; q < t.n_groups; ++q) {
    int64_t first, count;      // at most 240 + G slices in all
    group_units(t, q, L, first, count);
    a.first[q] = (int)first; a.count[q] = (int)count;
  }
  const int n = (p0.rows * (p0.cols + 1) + p1.rows * (p1.cols + 1)) * t.n_groups;      // at most 4 x 1872 x 73
  hipLaunchKernelGGL(slice_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

// one thread per (node, column), columns along lanes: a row is read as one coalesced piece, order[k] is the same address for the lanes of a node.  MEAN: a
// true division, as torch_scatter's
template <bool MEAN>
__global__ __launch_bounds__(256) void seg_kernel(const float* __restrict__ rows, const int32_t* __restrict__ order, const int64_t* __restrict__ ptr,
                                                  float* __restrict__ nodes, int64_t N, int D) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * D) return;
  const int64_t n = idx / D;
  const int c = (int)(idx - n * D);
  const int64_t k0 = ptr[n], k1 = ptr[n + 1];
  float sum = 0.f;
  int64_t k = k0;
  if (k < k1) sum = rows[(int64_t)order[k++] * D + c];      // (not 0 + row: a -0 stays what it is)
  for (; k + 4 <= k1; k += 4) {      // four loads in flight, added in order
    const float v0 = rows[(int64_t)order[k] * D + c], v1 = rows[(int64_t)order[k + 1] * D + c];
    const float v2 = rows[(int64_t)order[k + 2] * D + c], v3 = rows[(int64_t)order[k + 3] * D + c];
    sum += v0; sum += v1; sum += v2; sum += v3;
  }
  for (; k < k1; ++k) sum += rows[(int64_t)order[k] * D + c];
  if (MEAN) sum = sum / (float)(k1 - k0 > 1 ? k1 - k0 : 1);
  nodes[idx] = sum;
}

template <bool MEAN>
static hipError_t seg_launch(const float* rows, const int32_t* order, const int64_t* ptr, float* nodes, int64_t N, int D, hipStream_t s) {
  const int64_t nb = (N * D + 255) / 256;      // N < 2^31 and D <= 128: fewer than 2^31 workgroups
  if (nb > 0) hipLaunchKernelGGL((seg_kernel<MEAN>), dim3((unsigned)nb), dim3(256), 0, s, rows, order, ptr, nodes, N, D);
  return hipGetLastError();
}

hipError_t launch_seg_sum(const float* rows, const int32_t* order, const int64_t* ptr, float* nodes, int64_t N, int D, hipStream_t s) {
  return seg_launch<false>(rows, order, ptr, nodes, N, D, s);
}
hipError_t launch_seg_mean(const float* rows, const int32_t* order, const int64_t* ptr, float* nodes, int64_t N, int D, hipStream_t s) {
  return seg_launch<true>(rows, order, ptr, nodes, N, D, s);
}

}  // namespace ddk
