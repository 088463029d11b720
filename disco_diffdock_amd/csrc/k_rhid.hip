// The first half of a conv layer's radial MLP at the op boundary, and its vector-Jacobian product, WITHOUT the concatenated row [E, 72]:
//   pre_e = W1[g(e)] [ emb_e | xs[src_e] | xs[dst_e] ] + b1[g(e)]      h_e = dropout(relu(pre_e))      (models/score_model.py:227-230 and fc[g][0..3] of
// models/tensor_layers.py:154).  The row is gathered inside the kernels; the backward adds the two gathers' gradients per node in ascending edge id (the
// fixed-order segmented sum of k_reduce.hip), so nothing here uses an atomic and the bits do not depend on the run, the device or the
// subset of gradients asked for.  Exact fp32: every dot product is ONE fmaf chain in a written-out order (compiled with -ffp-contract=off, so that the
// only fused operations are the ones spelled fmaf):
//   pre[e, c]   = fmaf(W1[c, 71], in[71], ... fmaf(W1[c, 0], in[0], b1[c]))                     k ascending, the bias first
//   gin[e, k]   = fmaf(gpre[71], W1[71, k], ... fmaf(gpre[0], W1[0, k], 0))                     c ascending
//   grad_W1[c, k] = the slices' partial sums added in slice order, a partial sum being fmaf(gpre[e, c], in[e, k], .) over the slice's edges ascending
//   h[e, c]     = pre < 0 ? 0 : pre at p == 0; keep(e, c) ? (pre < 0 ? 0 : pre) * s : 0 otherwise, s = 1.0f / (1.0f - p) formed once on the host in fp32
//   gpre[e, c]  = grad_h[e, c] * (h[e, c] != 0 ? s : 0): one product
//   grad_b1[c]  = as grad_W1 with a separate add, acc += gpre[e, c], in place of the fmaf.  Every partial sum and every sum over the slices starts from +0
//                 (sum = 0; sum += image[s]); a group's slices are rtp_slice_len(E) edges each, counted from the group's first edge
//   grad_xs[n]  = (the node's src rows added in ascending edge id) + (its dst rows likewise): two segmented sums of k_reduce.hip, then one add in that order
//
// LAYOUT.  One LANE owns one EDGE, and a step walks FOUR COLUMNS of W1[g] (all 72 rows of them: 72 loads of 16 bytes).  Forward: the lane's 72
// accumulators sit in registers and start from the bias, its gathered row waits in LDS and gives the step's four inputs.  Backward: the lane's gpre row
// sits in 72 registers and the step makes four columns of gin.  A workgroup is two waves = 128 edges of ONE group, so what a step reads of W1 is the same
// address in every lane: the compiler reads it with scalar loads through the constant cache (W1[g] is 20.7 KB and is shared by every workgroup of the
// group) and v_fmac_f32 takes it from the scalar register; the vector ALU does little but the 72 x 72 fused multiply-adds of its edge.  A lane's row and
// its results live in an LDS tile [64][73] of its wave (stride 73: the lanes of an access hit 64 different banks); the results leave it as whole rows,
// coalesced, and these are the only global stores of the edge kernels: none comes before the last read of W1.  (A backward that sends its three parts
// through a tile [64][25], for four waves per SIMD instead of two, was measured and is no faster: the step's 72 scalar loads bound it, not occupancy.)
//
// THE MASK (include/ddk.h, DDK_RHID_MASK_LAYOUT): keep(e, c) = rng_uniform(word c % 4 of Philox4x32-10(key = seed, counter = (e_lo, e_hi, c / 4,
// DDK_RHID_MASK_TAG))) >= p: a pure function of (seed, edge id, column).  One block per four columns of h; drawn after the GEMM, into the lane's row of
// the tile, whose inputs are used up.  The backward reads the pattern from h itself (h != 0), so it needs neither the seed nor a mask tensor.
//
// rhid_param_kernel + the slice reduction of k_reduce.hip, as rtp_param_kernel: a workgroup of twelve waves owns an edge slice of a group and keeps the
// slice's image [72][73] in registers (a half-wave owns three columns, its lane three rows: 3 x 3 accumulators; column 72, the sum of gpre itself, is
// grad_b1) while 32 edges at a time are staged in LDS, gpre [32][72] and the gathered rows [32][72]: grad_h and h are read once, and a thread loads
// its elements of the next step into registers before it makes this step's products.  Plain stores; the
// second kernel adds a group's images in slice order.  The slice length is rtp_slice_len(E), a function of E alone, which also bounds the workgroups
// (240 + G): hence the twelve waves each.
#include "ddk_internal.h"
#include "k_philox.h"

namespace ddk {

constexpr int RH_W = 72;             // width of the concatenated row and of the hidden layer (3 ns)
constexpr int RH_P = 24;             // one part of the row: emb, xs[src] or xs[dst] (ns)
constexpr int RH_EPB = 128;          // edges per workgroup of the edge kernels: two waves, one edge per lane
constexpr int RH_LD = RH_W + 1;      // row stride of a wave's LDS tile
constexpr int RH_IMG = RH_W + 1;     // columns of a partial image: grad_w1's 72 and grad_b1
static_assert(RH_W == NE && RH_P == NS, "the radial MLP of ns = 24");

struct RhidArgs {
  const float* xs; const float* emb; const float* h; const float* gh;
  const int32_t* src; const int32_t* dst;
  float* out_h; float* gemb; float* rows_src; float* rows_dst; float* img;
  EdgeGroupTable t;
  int64_t L;      // edges per slice (parameter pass)
  float p, s;
  uint32_t seed_lo, seed_hi;
};

__device__ __forceinline__ void rhid_load24(const float* row, bool on, float* v) {
#pragma unroll
  for (int q = 0; q < RH_P / 4; ++q) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) t = reinterpret_cast<const float4*>(row)[q];
    v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
  }
}

// gpre = grad_h * (h != 0 ? s : 0): the one expression of it, in the edge kernel and in the parameter kernel
__device__ __forceinline__ float rhid_gpre(float gh, float h, float s) { return gh * (h != 0.f ? s : 0.f); }

// ---- forward -------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RH_EPB) void rhid_fwd_kernel(RhidArgs a, const float* __restrict__ w1, const float* __restrict__ b1) {
  __shared__ float tile[RH_EPB / 64][64 * RH_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const GroupUnit u = group_unit(a.t, blockIdx.x, RH_EPB);
  if (u.grp < 0) return;      // (the whole workgroup)
  const int64_t e0 = u.begin + 64 * wave, e = e0 + lane;
  const bool ev = e < u.end;
  // the lane's gathered row waits in its row of the tile: the 72 registers hold the accumulators, and a step reads four columns of the row
  float* t = tile[wave] + lane * RH_LD;
  {
    float in[RH_W];
    rhid_load24(a.emb + e * RH_P, ev, in);
    rhid_load24(a.xs + (int64_t)(ev ? a.src[e] : 0) * RH_P, ev, in + RH_P);
    rhid_load24(a.xs + (int64_t)(ev ? a.dst[e] : 0) * RH_P, ev, in + 2 * RH_P);
#pragma unroll
    for (int k = 0; k < RH_W; ++k) t[k] = in[k];
  }
  const float* wg = w1 + (int64_t)u.grp * RH_W * RH_W;
  const float* bg = b1 + (int64_t)u.grp * RH_W;
  float acc[RH_W];
#pragma unroll
  for (int c = 0; c < RH_W; ++c) acc[c] = bg[c];
#pragma unroll 1
  for (int k = 0; k < RH_W; k += 4) {      // columns k .. k + 3 of every row of W1[g]: for each output the chain runs over k in ascending order
    float x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = t[k + i];
#pragma unroll
    for (int c = 0; c < RH_W; ++c) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[c] = fmaf(wg[c * RH_W + k + i], x[i], acc[c]);
    }
  }
  if (a.p > 0.f) {
#pragma unroll 1
    for (int q = 0; q < RH_W / 4; ++q) {      // the mask goes to the tile as 1 / 0 (the row's inputs are used up)
      const MaskKeep4 keep = mask_keep4(a.seed_lo, a.seed_hi, e, q, DDK_RHID_MASK_TAG, a.p);
#pragma unroll
      for (int i = 0; i < 4; ++i) t[4 * q + i] = keep[i] ? 1.f : 0.f;
    }
#pragma unroll
    for (int c = 0; c < RH_W; ++c) t[c] = mask_relu(t[c] != 0.f, acc[c], a.s);
  } else {
#pragma unroll
    for (int c = 0; c < RH_W; ++c) t[c] = acc[c] < 0.f ? 0.f : acc[c];
  }
  __syncthreads();
  if (e0 < u.end) {
    const int n_e = u.end - e0 < 64 ? (int)(u.end - e0) : 64;
    for (int f = lane; f < n_e * RH_W; f += 64) {
      const int r = f / RH_W;
      a.out_h[e0 * RH_W + f] = tile[wave][r * RH_LD + (f - r * RH_W)];
    }
  }
}

// ---- backward, per edge: grad_emb rows and the per-edge rows of the two gathers' gradients ---------------------------------------------------------------------
__global__ __launch_bounds__(RH_EPB) void rhid_bwd_edge_kernel(RhidArgs a, const float* __restrict__ w1) {
  __shared__ float tile[RH_EPB / 64][64 * RH_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const GroupUnit u = group_unit(a.t, blockIdx.x, RH_EPB);
  if (u.grp < 0) return;
  const int64_t e0 = u.begin + 64 * wave, e = e0 + lane;
  const bool ev = e < u.end;
  float gp[RH_W];
#pragma unroll
  for (int q = 0; q < RH_W / 4; ++q) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), hv = g;
    if (ev) {
      g = reinterpret_cast<const float4*>(a.gh + e * RH_W)[q];
      hv = reinterpret_cast<const float4*>(a.h + e * RH_W)[q];
    }
    gp[4 * q] = rhid_gpre(g.x, hv.x, a.s); gp[4 * q + 1] = rhid_gpre(g.y, hv.y, a.s);
    gp[4 * q + 2] = rhid_gpre(g.z, hv.z, a.s); gp[4 * q + 3] = rhid_gpre(g.w, hv.w, a.s);
  }
  const float* wg = w1 + (int64_t)u.grp * RH_W * RH_W;
  float* t = tile[wave] + lane * RH_LD;
  const int k0 = a.gemb ? 0 : RH_P, k1 = a.rows_src ? RH_W : RH_P;      // the columns asked for: each is the same chain whatever else is computed
#pragma unroll 1
  for (int k = k0; k < k1; k += 4) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < RH_W; ++c) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(gp[c], wg[c * RH_W + k + i], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) t[k + i] = acc[i];
  }
  __syncthreads();
  if (e0 < u.end) {
    const int n_e = u.end - e0 < 64 ? (int)(u.end - e0) : 64;
#pragma unroll
    for (int part = 0; part < 3; ++part) {
      float* to = part == 0 ? a.gemb : (part == 1 ? a.rows_src : a.rows_dst);
      if (!to) continue;
      for (int f = lane; f < n_e * RH_P; f += 64) {
        const int r = f / RH_P;
        to[e0 * RH_P + f] = tile[wave][r * RH_LD + RH_P * part + (f - r * RH_P)];
      }
    }
  }
}

// ---- backward, parameters --------------------------------------------------------------------------------------------------------------------------------------
constexpr int RH_PT = 768;      // threads of rhid_param_kernel: 24 half-waves of three columns each

__global__ __launch_bounds__(RH_PT) void rhid_param_kernel(RhidArgs a) {
  __shared__ float gps[32 * RH_W];
  __shared__ float ins[32 * RH_W];
  const int tid = threadIdx.x, tc = tid & 31, tk = tid >> 5;      // rows 3 tc .. 3 tc + 2 (tc < 24) x columns 3 tk .. 3 tk + 2
  const int64_t slice = blockIdx.x;
  const GroupUnit u = group_unit(a.t, slice, a.L);
  if (u.grp < 0) return;
  const bool active = tc < RH_P;
  float acc[3][3], accb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    accb[i] = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = 0.f;
  }
  // the thread's three elements of gpre and of the gathered rows of the 32 edges from eb on: loaded one step ahead, so that the loads of the next step
  // are in flight while this one's products are made
  constexpr int NF = 32 * RH_W / RH_PT;
  static_assert(NF * RH_PT == 32 * RH_W, "every thread stages the same number of elements");
  float gv[NF], xv[NF];
  auto fetch = [&](int64_t eb) {
    const int n_e = u.end - eb < 32 ? (int)(u.end - eb) : 32;
#pragma unroll
    for (int q = 0; q < NF; ++q) {
      const int f = tid + q * RH_PT, r = f / RH_W, col = f - r * RH_W;
      gv[q] = 0.f; xv[q] = 0.f;
      if (r < n_e) {
        gv[q] = rhid_gpre(a.gh[eb * RH_W + f], a.h[eb * RH_W + f], a.s);
        const int part = col / RH_P;
        xv[q] = part == 0 ? a.emb[(eb + r) * RH_P + col] : a.xs[(int64_t)(part == 1 ? a.src[eb + r] : a.dst[eb + r]) * RH_P + (col - part * RH_P)];
      }
    }
  };
  fetch(u.begin);
  for (int64_t eb = u.begin; eb < u.end; eb += 32) {
    __syncthreads();      // (the step before is done with the two images)
#pragma unroll
    for (int q = 0; q < NF; ++q) { gps[tid + q * RH_PT] = gv[q]; ins[tid + q * RH_PT] = xv[q]; }
    __syncthreads();
    if (eb + 32 < u.end) fetch(eb + 32);
    if (active) {
#pragma unroll 4
      for (int el = 0; el < 32; ++el) {      // the edges past n_e are staged as zeros: they leave every sum as it is
        float g[3], x[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { g[i] = gps[el * RH_W + 3 * tc + i]; x[i] = ins[el * RH_W + 3 * tk + i]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          accb[i] += g[i];
#pragma unroll
          for (int j = 0; j < 3; ++j) acc[i][j] = fmaf(g[i], x[j], acc[i][j]);
        }
      }
    }
  }
  if (active) {
    float* img = a.img + slice * (int64_t)(RH_W * RH_IMG);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) img[(3 * tc + i) * RH_IMG + 3 * tk + j] = acc[i][j];
      if (tk == 0) img[(3 * tc + i) * RH_IMG + RH_W] = accb[i];
    }
  }
}

// grad_xs = (the sum over the node's edges as src) + (the sum over its edges as dst), in that order
__global__ __launch_bounds__(256) void rhid_add_kernel(float* __restrict__ to, const float* __restrict__ add, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < n) to[idx] = to[idx] + add[idx];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------
int64_t rhid_workspace(int64_t E, int32_t n_groups, int64_t n_nodes) {
  const int64_t lim = (int64_t)1 << 31;
  if (E < 0 || E >= lim || n_groups < 1 || n_groups > 4 || n_nodes < 0 || n_nodes >= lim) return -1;
  return (2 * ws_pad(E * RH_P) + ws_pad(n_nodes * RH_P) + slice_bound(E, n_groups) * RH_W * RH_IMG) * (int64_t)sizeof(float);
}

static RhidArgs rhid_args(const float* xs, const int32_t* src, const int32_t* dst, const float* emb, const int64_t* group_offsets, int n_groups, float p) {
  RhidArgs a{};
  a.xs = xs; a.src = src; a.dst = dst; a.emb = emb;
  a.t = group_table(group_offsets, n_groups);
  a.L = rtp_slice_len(group_offsets[n_groups]);
  a.p = p;
  a.s = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
  return a;
}

hipError_t launch_rhid_forward(const float* xs, const int32_t* src, const int32_t* dst, const float* emb, const int64_t* group_offsets, int n_groups,
                               const float* w1, const float* b1, float p, uint64_t seed, float* h, hipStream_t s) {
  if (group_offsets[n_groups] == 0) return hipSuccess;
  RhidArgs a = rhid_args(xs, src, dst, emb, group_offsets, n_groups, p);
  a.out_h = h;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
  const int64_t nwg = group_unit_total(a.t, RH_EPB);      // E < 2^31: fewer than 2^31 workgroups
  hipLaunchKernelGGL(rhid_fwd_kernel, dim3((unsigned)nwg), dim3(RH_EPB), 0, s, a, w1, b1);
  return hipGetLastError();
}

hipError_t launch_rhid_backward(const RconvGraph& gr, const float* xs, const float* emb, const float* h, const int64_t* group_offsets, int n_groups,
                                const float* w1, const float* grad_h, float p, float* grad_xs, float* grad_emb, float* grad_w1, float* grad_b1,
                                float* workspace, hipStream_t s) {
  const int64_t E = group_offsets[n_groups], N = gr.n_in;
  if (E == 0) {
    hipError_t e = zero_async(grad_xs, N * RH_P, s);
    if (e == hipSuccess) e = zero_async(grad_w1, (int64_t)n_groups * RH_W * RH_W, s);
    if (e == hipSuccess) e = zero_async(grad_b1, (int64_t)n_groups * RH_W, s);
    return e;
  }
  float* rows_src = workspace;
  float* rows_dst = rows_src + ws_pad(E * RH_P);
  float* node_dst = rows_dst + ws_pad(E * RH_P);
  RhidArgs a = rhid_args(xs, gr.src, gr.dst, emb, group_offsets, n_groups, p);
  a.h = h; a.gh = grad_h;
  a.gemb = grad_emb; a.rows_src = grad_xs ? rows_src : nullptr; a.rows_dst = grad_xs ? rows_dst : nullptr;
  a.img = node_dst + ws_pad(N * RH_P);
  hipError_t e = hipSuccess;
  if (grad_emb || grad_xs) {
    hipLaunchKernelGGL(rhid_bwd_edge_kernel, dim3((unsigned)group_unit_total(a.t, RH_EPB)), dim3(RH_EPB), 0, s, a, w1);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (grad_xs) {
    if ((e = launch_seg_sum(rows_src, gr.src_order, gr.src_ptr, grad_xs, N, RH_P, s)) != hipSuccess) return e;
    if ((e = launch_seg_sum(rows_dst, gr.dst_order, gr.dst_ptr, node_dst, N, RH_P, s)) != hipSuccess) return e;
    const int64_t n = N * RH_P;      // N < 2^31: fewer than 2^31 workgroups
    hipLaunchKernelGGL(rhid_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, grad_xs, node_dst, n);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (grad_w1 || grad_b1) {
    hipLaunchKernelGGL(rhid_param_kernel, dim3((unsigned)group_unit_total(a.t, a.L)), dim3(RH_PT), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = launch_slice_reduce(a.img, a.t, a.L, ReducePart{grad_w1, grad_b1, RH_W, RH_W}, ReducePart{}, s);
  }
  return e;
}

}  // namespace ddk
