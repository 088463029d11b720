// The AR latent model's loss (include/ddk.h: ddk_node_cross_entropy_batch): the reference's per-graph loop of F.cross_entropy calls over a graph's ligand and
// receptor nodes (autoregressive/train_ar.py:116-127, 152-177) for a whole collated batch in one launch.  ONE WORKGROUP of 256 threads per graph; the class
// axis is the graph's ligand nodes, then its receptor nodes, position p = 0 .. n_lig_g + n_rec_g - 1, as in k_gumbel.hip, whose pointer-pair rule and
// summation order this file shares.  s_p: the student's logit (one column); t_p: column c = column[g] of the teacher's tables [., D].  A written-out order
// (compiled with -ffp-contract=off), every reduction in fp64:
//   m_s   = max s_p, pick = the LOWEST p with s_p = m_s;   m_t = max t_p, target = the LOWEST p with t_p = m_t   (no p above -inf, or NaN only: position 0)
//   lse_s = m_s + log(sum exp(s_p - m_s))                   thread t adds its positions (quads t, t + 256, ... of four positions, ascending) to a partial that
//                                                           starts from 0, the 256 partials are added by the fixed halving tree
//   hard  (soft = 0): q = target, loss = fl32(lse_s - s_q)
//   soft  (soft = 1): lse_t as lse_s, p_t = exp(t_p - lse_t), loss = fl32(lse_s - sum p_t s_p), the sum in the same order
// saved per graph for the backward: (lse_s, lse_t) as fp64, with pick and target; never anything per node.  The backward is element-wise:
//   grad_logit_p = grad_g * (fl32(exp(s_p - lse_s)) - target_p)   in fp32, target_p = [p == q] (hard) or fl32(exp(t_p - lse_t)) (soft)
// No atomics, no scratch, no node limit.  A graph whose pointer pair is no range of its table, whose column is outside 0 .. D - 1 or that has no node is
// left alone: none of its outputs is written, in either direction.
#include "ddk_internal.h"

namespace ddk {

constexpr int NCE_T = 256;

// the graph's nodes on both sides and its teacher column, or n < 0 where a pointer pair is no range of its table or the column none of the teacher's
struct NodeCeGraph { int64_t l0, r0, nl, n; int c; };
template <class Args>
__device__ __forceinline__ NodeCeGraph node_ce_graph(const Args& a, int g) {
  const int64_t l0 = a.lig_ptr[g], l1 = a.lig_ptr[g + 1], r0 = a.rec_ptr[g], r1 = a.rec_ptr[g + 1];
  const int c = a.column[g];
  const bool ok = l0 >= 0 && l0 <= l1 && l1 <= a.n_lig && r0 >= 0 && r0 <= r1 && r1 <= a.n_rec && c >= 0 && c < a.D;
  return NodeCeGraph{l0, r0, l1 - l0, ok ? (l1 - l0) + (r1 - r0) : -1, c};
}
// position p of the graph: its student logit and the element of its teacher column
template <class Args>
__device__ __forceinline__ void node_ce_at(const Args& a, const NodeCeGraph& G, int64_t p, double& s, double& t) {
  const bool lig = p < G.nl;
  const int64_t row = lig ? G.l0 + p : G.r0 + (p - G.nl);
  s = (double)(lig ? a.s_l : a.s_r)[row];
  t = (double)(lig ? a.t_l : a.t_r)[row * a.D + G.c];
}

__device__ __forceinline__ double node_ce_tree_sum(double* red, double v) {
  const int t = threadIdx.x;
  __syncthreads();      // (the tile may still be read from the reduction before)
  red[t] = v;
  __syncthreads();
  for (int s = NCE_T / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = red[t] + red[t + s];
    __syncthreads();
  }
  return red[0];
}

// the maximum over the workgroup and the lowest position that holds it; a graph in which no position beats -inf answers position 0
__device__ __forceinline__ double node_ce_tree_max(double* red, int64_t* redi, double v, int64_t& where) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v; redi[t] = where;
  __syncthreads();
  for (int s = NCE_T / 2; s > 0; s >>= 1) {
    if (t < s) {
      const double o = red[t + s];
      const int64_t oi = redi[t + s];
      if (o > red[t] || (o == red[t] && oi < redi[t])) { red[t] = o; redi[t] = oi; }
    }
    __syncthreads();
  }
  where = redi[0] == INT64_MAX ? 0 : redi[0];
  return red[0];
}

__global__ __launch_bounds__(NCE_T) void node_ce_fwd_kernel(NodeCeArgs a) {
  __shared__ double red[NCE_T];
  __shared__ int64_t redi[NCE_T];
  const int g = blockIdx.x, t = threadIdx.x;
  const NodeCeGraph G = node_ce_graph(a, g);
  if (G.n <= 0) return;
  const int64_t quads = (G.n + 3) >> 2;
  // 1. both maxima and where they are first reached
  double ms = -INFINITY, mt = -INFINITY;
  int64_t ws = INT64_MAX, wt = INT64_MAX;
  for (int64_t q = t; q < quads; q += NCE_T) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t p = 4 * q + i;
      if (p < G.n) {
        double s, tt;
        node_ce_at(a, G, p, s, tt);
        if (s > ms) { ms = s; ws = p; }      // (ascending p: the first of equals stays)
        if (tt > mt) { mt = tt; wt = p; }
      }
    }
  }
  ms = node_ce_tree_max(red, redi, ms, ws);
  mt = node_ce_tree_max(red, redi, mt, wt);
  // 2. the two log-sum-exps
  double ps = 0.0, pt = 0.0;
  for (int64_t q = t; q < quads; q += NCE_T) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t p = 4 * q + i;
      if (p < G.n) {
        double s, tt;
        node_ce_at(a, G, p, s, tt);
        ps += exp(s - ms);
        if (a.soft) pt += exp(tt - mt);
      }
    }
  }
  const double lse_s = ms + log(node_ce_tree_sum(red, ps));
  const double lse_t = a.soft ? mt + log(node_ce_tree_sum(red, pt)) : 0.0;
  // 3. the label's term
  double term;
  if (a.soft) {
    double part = 0.0;
    for (int64_t q = t; q < quads; q += NCE_T) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t p = 4 * q + i;
        if (p < G.n) {
          double s, tt;
          node_ce_at(a, G, p, s, tt);
          part += exp(tt - lse_t) * s;
        }
      }
    }
    term = node_ce_tree_sum(red, part);
  } else {
    double tt;
    node_ce_at(a, G, wt, term, tt);
  }
  if (t == 0) {
    a.loss[g] = (float)(lse_s - term);
    a.pick[g] = ws;
    a.target[g] = wt;
    a.saved[2 * g] = lse_s;
    a.saved[2 * g + 1] = lse_t;
  }
}

__global__ __launch_bounds__(NCE_T) void node_ce_bwd_kernel(NodeCeBwdArgs a) {
  const int g = blockIdx.x, t = threadIdx.x;
  const NodeCeGraph G = node_ce_graph(a, g);
  if (G.n <= 0) return;
  const float go = a.grad[g];
  const double lse_s = a.saved[2 * g], lse_t = a.saved[2 * g + 1];
  const int64_t hit = a.target[g];
  for (int64_t p = t; p < G.n; p += NCE_T) {
    const bool lig = p < G.nl;
    const int64_t row = lig ? G.l0 + p : G.r0 + (p - G.nl);
    const float e = (float)exp((double)(lig ? a.s_l : a.s_r)[row] - lse_s);
    float label = p == hit ? 1.f : 0.f;
    if (a.soft) label = (float)exp((double)(lig ? a.t_l : a.t_r)[row * a.D + G.c] - lse_t);      // (hard mode reads no teacher table)
    (lig ? a.grad_l : a.grad_r)[row] = go * (e - label);
  }
}

hipError_t launch_node_ce_forward(const NodeCeArgs& a, int G, hipStream_t s) {
  hipLaunchKernelGGL(node_ce_fwd_kernel, dim3((unsigned)G), dim3(NCE_T), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_node_ce_backward(const NodeCeBwdArgs& a, int G, hipStream_t s) {
  hipLaunchKernelGGL(node_ce_bwd_kernel, dim3((unsigned)G), dim3(NCE_T), 0, s, a);
  return hipGetLastError();
}

}  // namespace ddk
