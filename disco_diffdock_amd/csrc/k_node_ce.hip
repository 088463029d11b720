// The AR latent model's loss (include/ddk.h: ddk_node_cross_entropy_batch): the reference's per-graph loop of F.cross_entropy calls over a graph's ligand and
// receptor nodes (autoregressive/train_ar.py:116-127, 152-177) for a whole collated batch in one launch.  ONE WORKGROUP of 256 threads per graph; the class
// axis is the graph's ligand nodes, then its receptor nodes, position p = 0 .. n_lig_g + n_rec_g - 1: the pointer-pair rule, the walk over the
// positions and the halving trees are k_ragged.h's, shared with k_gumbel.hip.  s_p: the student's logit (one column); t_p: column c = column[g] of the teacher's tables [., D].  A written-out order
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
#include "k_ragged.h"

namespace ddk {

// the graph's nodes on both sides and its teacher column c, n < 0 also where the column is none of the teacher's
template <class Args>
__device__ __forceinline__ RaggedGraph node_ce_graph(const Args& a, int g, int& c) {
  RaggedGraph G = ragged_graph(a.r.lig_ptr, a.r.rec_ptr, a.r.n_lig, a.r.n_rec, g);
  c = a.column[g];
  if (c < 0 || c >= a.r.D) G.n = -1;
  return G;
}
// position p of the graph: its student logit and the element of its teacher column
__device__ __forceinline__ void node_ce_at(const NodeCeArgs& a, const RaggedGraph& G, int c, int64_t p, double& s, double& t) {
  bool lig;
  const int64_t row = ragged_row(G, p, lig);
  s = (double)(lig ? a.s_l : a.s_r)[row];
  t = (double)(lig ? a.t_l : a.t_r)[row * a.r.D + c];
}

__global__ __launch_bounds__(RAGGED_T) void node_ce_fwd_kernel(NodeCeArgs a) {
  __shared__ double red[RAGGED_T];
  __shared__ int64_t redi[RAGGED_T];
  const int g = blockIdx.x;
  int c;
  const RaggedGraph G = node_ce_graph(a, g, c);
  if (G.n <= 0) return;
  double s, tt;
  // 1. both maxima and where they are first reached; a graph in which no position beats -inf answers position 0
  double ms = -INFINITY, mt = -INFINITY;
  int64_t ws = INT64_MAX, wt = INT64_MAX;
  ragged_for_each(G, [&](int64_t, int, int64_t p) {
    node_ce_at(a, G, c, p, s, tt);
    if (s > ms) { ms = s; ws = p; }      // (ascending p: the first of equals stays)
    if (tt > mt) { mt = tt; wt = p; }
  });
  ms = ragged_tree_argmax(red, redi, ms, ws);
  mt = ragged_tree_argmax(red, redi, mt, wt);
  if (ws == INT64_MAX) ws = 0;
  if (wt == INT64_MAX) wt = 0;
  // 2. the two log-sum-exps
  double ps = 0.0, pt = 0.0;
  ragged_for_each(G, [&](int64_t, int, int64_t p) {
    node_ce_at(a, G, c, p, s, tt);
    ps += exp(s - ms);
    if (a.soft) pt += exp(tt - mt);
  });
  const double lse_s = ms + log(ragged_tree_sum(red, ps));
  const double lse_t = a.soft ? mt + log(ragged_tree_sum(red, pt)) : 0.0;
  // 3. the label's term
  double term;
  if (a.soft) {
    double part = 0.0;
    ragged_for_each(G, [&](int64_t, int, int64_t p) {
      node_ce_at(a, G, c, p, s, tt);
      part += exp(tt - lse_t) * s;
    });
    term = ragged_tree_sum(red, part);
  } else {
    node_ce_at(a, G, c, wt, term, tt);
  }
  if (threadIdx.x == 0) {
    a.loss[g] = (float)(lse_s - term);
    a.pick[g] = ws;
    a.target[g] = wt;
    a.saved[2 * g] = lse_s;
    a.saved[2 * g + 1] = lse_t;
  }
}

__global__ __launch_bounds__(RAGGED_T) void node_ce_bwd_kernel(NodeCeBwdArgs a) {
  const int g = blockIdx.x;
  int c;
  const RaggedGraph G = node_ce_graph(a, g, c);
  if (G.n <= 0) return;
  const float go = a.grad[g];
  const double lse_s = a.saved[2 * g], lse_t = a.saved[2 * g + 1];
  const int64_t hit = a.target[g];
  for (int64_t p = threadIdx.x; p < G.n; p += RAGGED_T) {      // (element-wise: no quads, consecutive threads take consecutive rows)
    bool lig;
    const int64_t row = ragged_row(G, p, lig);
    const float e = (float)exp((double)(lig ? a.s_l : a.s_r)[row] - lse_s);
    float label = p == hit ? 1.f : 0.f;
    if (a.soft) label = (float)exp((double)(lig ? a.t_l : a.t_r)[row * a.r.D + c] - lse_t);      // (hard mode reads no teacher table)
    (lig ? a.grad_l : a.grad_r)[row] = go * (e - label);
  }
}

hipError_t launch_node_ce_forward(const NodeCeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(node_ce_fwd_kernel, dim3((unsigned)a.r.G), dim3(RAGGED_T), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_node_ce_backward(const NodeCeBwdArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(node_ce_bwd_kernel, dim3((unsigned)a.r.G), dim3(RAGGED_T), 0, s, a);
  return hipGetLastError();
}

}  // namespace ddk
