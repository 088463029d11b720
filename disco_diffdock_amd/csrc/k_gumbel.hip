// The ragged straight-through Gumbel softmax in front of the latent-conditioned score model (include/ddk.h: ddk_gumbel_softmax_batch, ddk_gumbel_pick_samples, DDK_GUMBEL_LAYOUT) and
// its vector-Jacobian product: the reference's per-graph loop (latent_encoder.py:328-335, pretrained_score_encoder.py:74-81 over models/layers.py:152-181) for a
// whole collated batch in one launch.  ONE WORKGROUP per (graph g, latent dimension d); the class axis is the graph's ligand nodes, then its receptor nodes,
// position p = 0 .. n_lig_g + n_rec_g - 1: the pointer-pair rule, the walk over the positions and the halving trees are k_ragged.h's, shared with
// k_node_ce.hip.  A written-out order (compiled with -ffp-contract=off):
//   u    = (word >> 8) * 2^-24                               the word of position p: see THE NOISE below
//   gum  = -log(-log(u + 1e-20f) + 1e-20)                    the addition to u in fp32, the rest in fp64
//   z    = (logit + gum) / T                                  in fp64, a true division; kept as the fp32 pair (hi, lo) with hi = fl32(z), lo = fl32(z - hi)
//   e    = fl32(exp(z - max z))                               in fp64 from the pairs, rounded once.  z is 1 / T times a number of the order of 10: at T = 0.01
//                                                             an fp32 z of 700 has an ulp of 6e-5, which every y under the winner's would carry as its RELATIVE
//                                                             error (tests/test_gpu_latent_choice_adversarial.py measured 6.5e-5 against an fp32 host's 1e-5)
//   y    = e / sum                                            in fp32.  The sum: thread t adds its positions (quads t, t + 256, ... of four positions, ascending)
//                                                             to a partial that starts from 0, then the 256 partials are added by the fixed halving tree
//   out  = (hard - y) + y                                     two operations as written; hard = 1 at the LOWEST position that holds the maximum of y, else 0
// and backward, from the saved y:  grad_logit = y * (g - sum g y) / T in fp32, the sum in the same order.  No atomics; between the passes y's buffer holds z's hi
// and then the exponentials, out's buffer z's lo (a thread reads back only what it wrote itself), so there is no limit on the number of nodes.
//
// THE NOISE (DDK_GUMBEL_LAYOUT 1): generator purpose 13 of DDK_RNG_LAYOUT 1, rng_block(seed, stream_id[g], sample, 13, draw, d), yields four words; words 0 and 1
// are the key of a second Philox4x32-10 whose counter (p / 4, 0, 0, DDK_GUMBEL_TAG) gives position p the word p % 4.  A graph's noise is a pure function of
// (seed, complex, sample, draw, d, position): the batch it sits in and its place there do not matter.
#include "ddk_internal.h"
#include "k_philox.h"
#include "k_ragged.h"

namespace ddk {

constexpr uint32_t RNG_GUMBEL = 13;      // DDK_RNG_LAYOUT 1, beside RngPurpose

struct GumbelArgs {      // the forward
  const float* logit_l; const float* logit_r;
  const int64_t* lig_ptr; const int64_t* rec_ptr; const uint64_t* stream_id;
  float* y_l; float* y_r; float* out_l; float* out_r;
  int64_t n_lig, n_rec;
  int D;
  float T;
  uint32_t seed_lo, seed_hi, sample, draw;
};
struct GumbelBwdArgs {      // the backward: the saved y and grad_out in, grad_logit out
  const float* y_l; const float* y_r; const float* gout_l; const float* gout_r;
  const int64_t* lig_ptr; const int64_t* rec_ptr;
  float* grad_l; float* grad_r;
  int64_t n_lig, n_rec;
  int D;
  float T;
};

// The forward of one (graph, latent dimension), the whole workgroup: the one body of gumbel_fwd_kernel and gumbel_pick_kernel.  The logits are read at the rows
// of ``in``, y and out are written at the rows of ``G`` (the same node counts; the ragged op passes one graph twice, the per-sample op the shared table and
// sample b's block of the outputs).  ``key``: rng_block's four words for (complex, sample, draw, d).  Returns the position of the one (n > 0 is the caller's),
// INT64_MAX where no y compares.
__device__ __forceinline__ int64_t gumbel_forward_body(const float* logit_l, const float* logit_r, float* y_l, float* y_r, float* out_l, float* out_r,
                                                       const RaggedGraph& in, const RaggedGraph& G, int D, int d, float T, const uint32_t* key) {
  __shared__ float red[RAGGED_T];
  __shared__ double redd[RAGGED_T];
  __shared__ int64_t redi[RAGGED_T];
  bool lig;
  // 1. z as (hi, lo) into y's and out's buffers, the thread's maximum of hi + lo
  double m = -INFINITY;
  uint32_t w[4];
  ragged_for_each(G, [&](int64_t q, int i, int64_t p) {
    if (i == 0) {      // (one Philox block per quad)
      const uint32_t ctr[4] = {(uint32_t)q, 0u, 0u, DDK_GUMBEL_TAG};
      philox4x32_10(ctr, key, w);
    }
    const int64_t at = ragged_row(G, p, lig) * D + d;
    const float u = rng_uniform(w[i]);
    const double gum = -log(-log((double)(u + 1e-20f)) + 1e-20);
    const double z = ((double)(lig ? logit_l : logit_r)[ragged_row(in, p, lig) * D + d] + gum) / (double)T;
    const float hi = (float)z, lo = isinf(hi) ? 0.f : (float)(z - (double)hi);
    (lig ? y_l : y_r)[at] = hi;
    (lig ? out_l : out_r)[at] = lo;
    m = fmax(m, (double)hi + (double)lo);
  });
  m = ragged_tree_fmax(redd, m);
  // 2. the exponentials and their sum
  float part = 0.f;
  ragged_for_each(G, [&](int64_t, int, int64_t p) {
    const int64_t at = ragged_row(G, p, lig) * D + d;
    float* y = lig ? y_l : y_r;
    const float e = (float)exp(((double)y[at] + (double)(lig ? out_l : out_r)[at]) - m);
    y[at] = e;
    part += e;
  });
  const float sum = ragged_tree_sum(red, part);
  // 3. y and the lowest position of its maximum
  float best = -INFINITY;
  int64_t where = INT64_MAX;
  ragged_for_each(G, [&](int64_t, int, int64_t p) {
    const int64_t at = ragged_row(G, p, lig) * D + d;
    float* y = lig ? y_l : y_r;
    const float v = y[at] / sum;
    y[at] = v;
    if (v > best) { best = v; where = p; }      // (ascending p: the first of equals stays)
  });
  ragged_tree_argmax(red, redi, best, where);
  // 4. the straight-through output
  ragged_for_each(G, [&](int64_t, int, int64_t p) {
    const int64_t at = ragged_row(G, p, lig) * D + d;
    const float y = (lig ? y_l : y_r)[at];
    const float hard = p == where ? 1.f : 0.f;
    (lig ? out_l : out_r)[at] = (hard - y) + y;
  });
  return where;
}

__global__ __launch_bounds__(RAGGED_T) void gumbel_fwd_kernel(GumbelArgs a) {
  const int g = blockIdx.x, d = blockIdx.y;
  const RaggedGraph G = ragged_graph(a.lig_ptr, a.rec_ptr, a.n_lig, a.n_rec, g);
  if (G.n <= 0) return;
  uint32_t key[4];
  rng_block(rng_stream(((uint64_t)a.seed_hi << 32) | a.seed_lo, a.stream_id[g]), a.sample, RNG_GUMBEL, a.draw, (uint32_t)d, key);
  gumbel_forward_body(a.logit_l, a.logit_r, a.y_l, a.y_r, a.out_l, a.out_r, G, G, a.D, d, a.T, key);
}

// ddk_gumbel_pick_samples: workgroup (b, d) is sample ``sample + b`` of ONE complex; every sample reads the one table of logits (rows 0 .. n - 1) and writes
// rows b n .. (b + 1) n - 1 of y (the context's scratch) and out.  stream_id is the complex id itself, by value; choices (or null) [B, D] takes the position of the
// one, ligand nodes first (-1 where no y compares: NaN logits).
struct GumbelPickArgs {
  const float* logit_l; const float* logit_r;
  float* y_l; float* y_r; float* out_l; float* out_r;
  int32_t* choices;
  int64_t n_lig, n_rec;
  uint64_t stream_id;
  int D;
  float T;
  uint32_t seed_lo, seed_hi, sample, draw;
};

__global__ __launch_bounds__(RAGGED_T) void gumbel_pick_kernel(GumbelPickArgs a) {
  const int b = blockIdx.x, d = blockIdx.y;
  const RaggedGraph in{0, 0, a.n_lig, a.n_lig + a.n_rec}, to{(int64_t)b * a.n_lig, (int64_t)b * a.n_rec, a.n_lig, a.n_lig + a.n_rec};
  uint32_t key[4];
  rng_block(rng_stream(((uint64_t)a.seed_hi << 32) | a.seed_lo, a.stream_id), a.sample + (uint32_t)b, RNG_GUMBEL, a.draw, (uint32_t)d, key);
  const int64_t where = gumbel_forward_body(a.logit_l, a.logit_r, a.y_l, a.y_r, a.out_l, a.out_r, in, to, a.D, d, a.T, key);
  if (a.choices && threadIdx.x == 0) a.choices[(int64_t)b * a.D + d] = (int32_t)where;
}

__global__ __launch_bounds__(RAGGED_T) void gumbel_bwd_kernel(GumbelBwdArgs a) {
  __shared__ float red[RAGGED_T];
  const int g = blockIdx.x, d = blockIdx.y;
  const RaggedGraph G = ragged_graph(a.lig_ptr, a.rec_ptr, a.n_lig, a.n_rec, g);
  if (G.n <= 0) return;
  bool lig;
  float part = 0.f;
  ragged_for_each(G, [&](int64_t, int, int64_t p) {
    const int64_t at = ragged_row(G, p, lig) * a.D + d;
    part += (lig ? a.gout_l : a.gout_r)[at] * (lig ? a.y_l : a.y_r)[at];
  });
  const float dot = ragged_tree_sum(red, part);
  ragged_for_each(G, [&](int64_t, int, int64_t p) {
    const int64_t at = ragged_row(G, p, lig) * a.D + d;
    const float y = (lig ? a.y_l : a.y_r)[at], go = (lig ? a.gout_l : a.gout_r)[at];
    (lig ? a.grad_l : a.grad_r)[at] = y * (go - dot) / a.T;
  });
}

hipError_t launch_gumbel_forward(const RaggedTables& o, float T, const float* logit_l, const float* logit_r, uint64_t seed, const uint64_t* stream_id, uint32_t sample,
                                 uint32_t draw, float* y_l, float* y_r, float* out_l, float* out_r, hipStream_t s) {
  GumbelArgs a{};
  a.logit_l = logit_l; a.logit_r = logit_r; a.lig_ptr = o.lig_ptr; a.rec_ptr = o.rec_ptr; a.stream_id = stream_id;
  a.y_l = y_l; a.y_r = y_r; a.out_l = out_l; a.out_r = out_r;
  a.n_lig = o.n_lig; a.n_rec = o.n_rec; a.D = o.D; a.T = T;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.sample = sample; a.draw = draw;
  hipLaunchKernelGGL(gumbel_fwd_kernel, dim3((unsigned)o.G, (unsigned)o.D), dim3(RAGGED_T), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_gumbel_pick(int B, int D, const float* logit_l, int64_t n_lig, const float* logit_r, int64_t n_rec, float T, uint64_t seed, uint64_t stream_id,
                              uint32_t sample0, uint32_t draw, float* y, float* out_l, float* out_r, int32_t* choices, hipStream_t s) {
  GumbelPickArgs a{};
  a.logit_l = logit_l; a.logit_r = logit_r; a.y_l = y; a.y_r = y + (int64_t)B * n_lig * D; a.out_l = out_l; a.out_r = out_r; a.choices = choices;
  a.n_lig = n_lig; a.n_rec = n_rec; a.stream_id = stream_id; a.D = D; a.T = T;
  a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.sample = sample0; a.draw = draw;
  hipLaunchKernelGGL(gumbel_pick_kernel, dim3((unsigned)B, (unsigned)D), dim3(RAGGED_T), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_gumbel_backward(const RaggedTables& o, float T, const float* y_l, const float* y_r, const float* gout_l, const float* gout_r, float* grad_l,
                                  float* grad_r, hipStream_t s) {
  const GumbelBwdArgs a{y_l, y_r, gout_l, gout_r, o.lig_ptr, o.rec_ptr, grad_l, grad_r, o.n_lig, o.n_rec, o.D, T};
  hipLaunchKernelGGL(gumbel_bwd_kernel, dim3((unsigned)o.G, (unsigned)o.D), dim3(RAGGED_T), 0, s, a);
  return hipGetLastError();
}

}  // namespace ddk
