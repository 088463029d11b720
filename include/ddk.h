/* ddk — C ABI of the MI355X-native DiffDock-S / DisCo-DiffDock-S score-model + sampler hot path.
 *
 * This is the drop-in boundary.  Every entry point names the reference
 * interface it replaces (paths relative to the reference checkout).  Conventions:
 *   - plain C, no torch types; all array arguments are CALLER-OWNED DEVICE pointers to
 *     contiguous row-major fp32 / int32 arrays unless the parameter is documented "host";
 *   - functions enqueue work on the given hipStream_t (passed as void*) and do not synchronise;
 *   - return 0 on success, a negative ddk_status otherwise; never throw across the ABI;
 *     ddk_last_error(ctx) returns a message for the last failure on that context;
 *   - a context is bound to one device, owns only its weight copies and workspaces, is not
 *     thread-safe, and holds no global state (one context per GPU / process).
 */
#ifndef DDK_H
#define DDK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ddk_ctx ddk_ctx;
typedef struct ddk_complex ddk_complex;

enum ddk_status {
  DDK_OK = 0,
  DDK_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
  DDK_ERR_HIP = -2,       /* a HIP runtime call failed */
  DDK_ERR_STATE = -3,     /* call order (e.g. weights not finalised) */
  DDK_ERR_NOMEM = -4
};

/* Constructor arguments of TensorProductScoreModel as utils/model_utils.py:25-68 (get_model) maps
 * them from model_parameters.yml, plus the ctor defaults it leaves alone (models/score_model.py:15-24)
 * and the diffusion constants t_to_sigma needs (utils/diffusion_utils.py:12-16). */
typedef struct ddk_config {
  int32_t ns, nv, num_conv_layers;
  int32_t sigma_embed_dim, distance_embed_dim, cross_distance_embed_dim;
  float lig_max_radius, rec_max_radius, cross_max_distance, center_max_distance;
  int32_t dynamic_max_cross;
  float embedding_scale;
  int32_t scale_by_sigma, no_torsion, batch_norm;
  int32_t latent_dim, latent_vocab;
  float latent_droprate;
  int32_t lm_embedding_dim;            /* 1280 when esm_embeddings_path is set, else 0 */
  float tr_sigma_min, tr_sigma_max, rot_sigma_min, rot_sigma_max, tor_sigma_min, tor_sigma_max;
  int32_t device;                      /* HIP device ordinal */
  /* all-atom confidence model (models/all_atom_score_model.py through get_model(..., confidence_mode=True)): */
  int32_t all_atoms;                   /* 1: AAScoreModel in confidence_mode (sh_lmax=2 FCTP, OldAtomEncoder, 9 convs/layer) */
  int32_t num_confidence_outputs;      /* len(rmsd_classification_cutoff)+1 when it is a list, else 1 */
  int32_t confidence_no_batchnorm;
  /* how the radial-MLP GEMMs (Linear(72,72) + ReLU + Linear(72,W), tensor_layers.py:140-143) of the fused conv kernel are multiplied.  Inputs, weights,
   * accumulators and outputs are fp32 in every mode; 0 and 3 run on the f16 matrix pipe with every fp32 operand carried as fp16 LIMBS (after an exact
   * power-of-two range scaling per weight group / per edge), 1 on the fp32 matrix pipe.
   *    The range-scaling groups: for the weights one whole fc.<g> matrix (W1 [72, 72]; W2 [W, 72] with the tensor product's 1/sqrt(fan-in) folded into its
   *    rows), scaled at pack time; for the activations one EDGE's 72 values (the GEMM1 inputs, then the hidden vector), scaled in the kernel.  A group's
   *    maximum lands in [2^14, 2^15).
   * 0 (default, since ddk 0.8): TWO limbs x = hi + mid (hi = fp16(x), mid = fp16(x - hi), both rounded to nearest) and the three limb products
   *    hi.hi + hi.mid + mid.hi in one fp32 accumulator (k_conv_x2.hip).  After scaling |x - hi - mid| <= max(2^-22 |x|, 2^-25): RELATIVE 2^-22 for every value
   *    within 17 binades of its range-scaling group's maximum, an ABSOLUTE 2^-39 of that maximum below (mid is then an fp16 subnormal).  Within the 17 binades
   *    the dropped mid.mid is <= 2^-22 relative like the operands' own truncation, the error per product <= 3 * 2^-22 relative, of a K = 72 dot product below the
   *    classical fp32 bound 72 * 2^-24 sum |a_i b_i| and, restated bit for bit on the host, not above an fp32 FMA chain's over the same operands
   *    (tests/test_limb_bound.py).  An output column whose weights all lie further under the largest weight of its matrix (or an edge whose activations lie further
   *    under its largest one) gets the absolute term instead: error <= 72 * 2^-24 sum |a_i b_i| + 2^-39 (max|W| sum |h_i| + max|h| sum |W_i|), pinned on
   *    adversarial operands per weight column by tests/test_gpu_conv_adversarial.py.  On randn operands it is level with mode 1 and mode 3 against the fp64
   *    oracle (6 - 10e-8 relative on every layer shape, tests/test_gpu_round6.py::test_two_limb_kernel_is_fp32_grade), 14 instead of 27 MFMAs per 32-edge
   *    weight tile.
   * 3: THREE limbs x = hi + mid + lo (exact for every value within 2^-15 of its range-scaling group's maximum, off by <= 2^-39 of that maximum below), six of the
   *    nine limb products kept (the dropped ones are <= 3 * 2^-33 relative), two fp32 accumulators (k_conv_x.hip): products exact to 2^-33 - the default of
   *    ddk 0.4 - 0.7, ~35 % more conv time than 0.
   * 1: v_mfma_f32_32x32x2_f32, plain fp32 FMA chains (k_conv.hip) - the stated fallback.  All three apply to the score model, its heads and the all-atom
   *    confidence model's conv layers.
   *    (Round 5's value 2 - a software-pipelined one-wave-per-SIMD form, measured 9 % slower - is refused: the kernel was removed, the last tree carrying it, under tools/variants/, is cd91202.) */
  int32_t conv_kernel;
  /* 1: fixed summation order per node in the score model's conv layers and heads (scatter_mean of tensor_layers.py:159): edges are
   *    sorted by the receiving node, so run tails STORE and the runs that straddle 32-edge tiles are folded in tile order by a second
   *    small kernel; one accumulator per (node, receiving edge group); no float atomics -> bit-identical outputs run to run.
   *    0 (default): wave-level segmented sums + fp32 atomics on the run tails (~1e-7 relative run-to-run noise).  Applies to
   *    ddk_score_forward / ddk_sample; ddk_conv_forward (caller-ordered edges) keeps the atomics; not with all_atoms. */
  int32_t deterministic;
  /* 1 (with all_atoms = 0): the coarse-grained model in confidence_mode - TensorProductScoreModel(confidence_mode=True) as
   *    get_model(args, ..., confidence_mode=True) builds it for a checkpoint without all_atoms (models/score_model.py:110-121, 186-189, 263-266):
   *    the score model's graph, embeddings and conv stack, complex_t used as sigma directly, no centre / torsion heads, a confidence_predictor
   *    on the pooled ligand scalars.  Evaluated by ddk_score_confidence; ddk_score_forward / ddk_sample refuse such a context. */
  int32_t confidence_mode;
} ddk_config;

/* ---- lifetime ---------------------------------------------------------------------------- */
int ddk_create(const ddk_config* cfg, ddk_ctx** out);
void ddk_destroy(ddk_ctx* ctx);
const char* ddk_last_error(ddk_ctx* ctx);
const char* ddk_version(void);

/* ---- checkpoint: replaces model.score_model.load_state_dict(state_dict, strict=True)
 *      (evaluate.py:169-171).  One call per state_dict tensor, HOST pointer, reference key name
 *      (e.g. "conv_layers.3.fc.2.4.weight").  Unknown "*.tp.*" buffer keys are ignored.
 *      ddk_finalize_weights checks that every required key arrived with the right shape and packs
 *      the radial-MLP weights into the MFMA fragment order the fused kernel streams. */
int ddk_load_weights(ddk_ctx* ctx, const char* name, const float* host_ptr, const int64_t* shape, int32_t ndim);
int ddk_finalize_weights(ddk_ctx* ctx);

/* Host tables of utils/so3.py:91-95 (_exp_score_norms, 1000 doubles) and utils/torus.py:79-83
 * (score_norm_, 5001 doubles; Monte-Carlo in the reference, shipped as data here). */
int ddk_set_score_norm_tables(ddk_ctx* ctx, const double* so3_exp_score_norms, int32_t n_so3,
                              const double* torus_score_norm, int32_t n_torus);

/* ---- a12: FasterTensorProduct.forward(in_, sh, weight)  models/tensor_layers.py:65-116.
 *      x_dst [E, Din] (already gathered node_attr[edge_dst]), sh [E,4], w [E, W] -> out [E, Dout]
 *      with the irreps of conv layer `layer` (0..num_conv_layers-1).  HBM-bound (streams w).
 *
 *      THE SECOND SHAPE FAMILY.  `layer` of the six tensor-product entries (ddk_tp_*, ddk_rtp_*, ddk_rconv_*) and of ddk_rtp_backward_workspace /
 *      ddk_rconv_workspace also takes DDK_TP_NV4 + l, l in 0..4: conv layer l of the ns = 24 / nv = 4 irreps sequence (get_irrep_seq(24, 4, False), the DisCo
 *      latent encoder's; 24x0e [+ 4x1o [+ 4x1e [+ 24x0o]]] -> the next entry; W = 672 / 800 / 928 / 1600 / 1600).  These ids name a shape, not a layer of
 *      the context: any finalised device context serves them, with or without weights.  A context with more than eight conv layers refuses the ids that
 *      are also indices of its own layers (DDK_ERR_INVALID; those layers have the shape of layer 3): an id is never reinterpreted.  The fused inference kernel (ddk_conv_forward) has no such ids. */
#define DDK_TP_NV4 8
/*      THE THIRD SHAPE FAMILY (the all-atom confidence model, sh_lmax = 2).  `layer` of ddk_rtp_*, ddk_rconv_*, ddk_rtp_backward_workspace and
 *      ddk_rconv_workspace also takes DDK_TP_AA + l, l in 0..4: conv layer l of models/all_atom_score_model.py, e3nn's
 *      FullyConnectedTensorProduct(in, 1x0e + 1x1o + 1x2e, out) on the irreps of the first family (Din 24 / 42 / 60 / 84, Dout 42 / 60 / 84 / 84;
 *      W = 720 / 972 / 1224 / 1944 / 1944).  For these ids
 *        - sh has 9 floats per edge, [Y0 | Y1 (3) | Y2 (5)] in e3nn's component order and 'component' normalisation (no alignment is asked of it); the
 *          op is bilinear in (x, sh, w) for any sh row;
 *        - a weight row is e3nn's: one [mul_in, mul_out] matrix per instruction, the instructions in the order (input irrep, sh irrep, output irrep),
 *          each path scaled by sqrt(dim_out / fan-in of its output) times the Frobenius-normalised Wigner 3j (layer 3: (0e,0e,0e) @ 0, (0e,1o,1o) @ 576,
 *          (1o,0e,1o) @ 720, (1o,1o,0e) @ 756, (1o,1o,1e) @ 900, (1o,2e,1o) @ 936, (1e,0e,1e) @ 972, (1e,1o,1o) @ 1008, (1e,1o,0o) @ 1044,
 *          (1e,2e,1e) @ 1188, (0o,0e,0o) @ 1224, (0o,1o,1e) @ 1800);
 *        - grad_sh is not implemented (poses are data where this model trains): a non-NULL grad_sh is DDK_ERR_INVALID;
 *        - ddk_tp_forward / ddk_tp_backward (per-edge weights [E, W]) refuse the ids by name: nothing in this model's training holds [E, 1944].
 *      Like DDK_TP_NV4 + l the ids name a shape, not a layer of the context (a context holds at most 16 conv layers, indices 0..15, so none of its own
 *      layers has such an index; one that did would be refused, not reinterpreted).  The same exact fp32 chains, no atomics, the same bits from run to
 *      run and whichever outputs are asked for. */
#define DDK_TP_AA 16
int ddk_tp_forward(ddk_ctx* ctx, int32_t layer, const float* x_dst, const float* sh, const float* w,
                   int64_t E, float* out, void* stream);

/* VJP of ddk_tp_forward.  All DEVICE pointers; no allocation, no synchronisation.  grad_x [E,Din], grad_sh [E,4], grad_w [E,W]: each may be NULL (not computed);
 * all three NULL is DDK_ERR_INVALID.  w may be NULL iff grad_x == grad_sh == NULL.  E == 0: DDK_OK, no launch.  Outputs must not alias inputs. */
int ddk_tp_backward(ddk_ctx* ctx, int32_t layer, const float* x_dst, const float* sh, const float* w, const float* grad_out, int64_t E,
                    float* grad_x, float* grad_sh, float* grad_w, void* stream);

/* ---- The radial tensor product of conv-layer shape `layer` (0..4, DDK_TP_NV4 + 0..4, or DDK_TP_AA + 0..4 with sh [E, 9]: see DDK_TP_AA): out[e] = FasterTensorProduct(x_dst[e], sh[e], w2[g(e)] h[e] + b2[g(e)]), the per-edge
 *      weights [E, W] never stored (models/tensor_layers.py:154-156 without the last Linear's output and the cat).  x_dst [E, Din], sh [E, 4], h [E, 72] (the
 *      radial MLP's hidden activation), w2 [n_groups, W, 72] and b2 [n_groups, W] (fc[g][4].weight / .bias stacked), out [E, Dout]: DEVICE pointers, fp32,
 *      contiguous.  group_offsets: HOST array of n_groups + 1 entries (n_groups in 1..4), 0 = o_0 <= ... <= o_G = E; edge e belongs to group g iff
 *      o_g <= e < o_{g+1}.  No allocation, no synchronisation.  E == 0: DDK_OK, no launch. */
int ddk_rtp_forward(ddk_ctx* ctx, int32_t layer, const float* x_dst, const float* sh, const float* h, const int64_t* group_offsets, int32_t n_groups,
                    const float* w2, const float* b2, int64_t E, float* out, void* stream);

/* VJP of ddk_rtp_forward.  grad_x [E, Din], grad_sh [E, 4], grad_h [E, 72], grad_w2 [n_groups, W, 72], grad_b2 [n_groups, W]: each may be NULL (not computed);
 * all five NULL is DDK_ERR_INVALID.  w2 and b2 may be NULL iff grad_x == grad_sh == grad_h == NULL (b2 is read for grad_x / grad_sh only: they need
 * w = w2 h + b2).  workspace: ddk_rtp_backward_workspace(layer, E, n_groups) bytes of device memory, needed only when grad_w2 or grad_b2 is asked for.
 * E == 0 and groups without edges: the grad_w2 / grad_b2 asked for are written as zeros.  Outputs must not alias inputs.  The same bits from call to call,
 * on every device, and whichever subset of the outputs is asked for. */
int ddk_rtp_backward(ddk_ctx* ctx, int32_t layer, const float* x_dst, const float* sh, const float* h, const int64_t* group_offsets, int32_t n_groups,
                     const float* w2, const float* b2, const float* grad_out, int64_t E, float* grad_x, float* grad_sh, float* grad_h, float* grad_w2,
                     float* grad_b2, void* workspace, void* stream);

/* Bytes of ddk_rtp_backward's workspace: a function of its arguments alone (never more than 160 MB); -1 for a layer outside 0..4, DDK_TP_NV4 + 0..4 and DDK_TP_AA + 0..4, n_groups outside 1..4,
 * E < 0 or E >= 2^31.  Host function, no context. */
int64_t ddk_rtp_backward_workspace(int32_t layer, int64_t E, int32_t n_groups);

/* ---- The radial conv of conv-layer shape `layer` (0..4), node features to aggregated node features: lines 153-159 of TensorProductConvLayer.forward with
 *      reduce='mean' (models/tensor_layers.py), the gather inside the radial tensor product's kernels and the scatter a fixed-order segmented sum:
 *        out_nodes[n] = (sum over the edges e with edge_src[e] == n, in ascending e, of FasterTensorProduct(x_nodes[edge_dst[e]], sh[e], w2[g(e)] h[e] + b2[g(e)]))
 *                       / max(number of those edges, 1)                     (a true division; a node without edges: exact zeros)
 *      x_nodes [n_in, Din], out_nodes [n_out, Dout]; edge_src, edge_dst: int32 [E], 0 <= edge_src < n_out, 0 <= edge_dst < n_in; src_order: int32 [E], the
 *      edge ids sorted by edge_src, ascending edge id within a node (a stable sort); src_ptr: int64 [n_out + 1], node n owns src_order[src_ptr[n] ..
 *      src_ptr[n + 1]).  sh, h, group_offsets, n_groups, w2, b2, E: as ddk_rtp_forward.  DEVICE pointers (group_offsets: HOST), fp32, contiguous; no allocation,
 *      no synchronisation.  The indices, orderings and pointer tables are TRUSTED (an index outside its range reads or writes outside the buffers): they must
 *      come from a validated graph, Context.conv_graph in Python.
 *      workspace: ddk_rconv_workspace(layer, E, n_groups, n_in, n_out, 0) bytes of device memory: the [E, Dout] rows of the tensor product and nothing else.
 *      Never stored: the per-edge weights [E, W], the gathered rows x_nodes[edge_dst] [E, Din].
 *      E == 0: out_nodes is written as zeros, no kernel of the tensor product is launched.  Outputs must not alias inputs.  No atomics: the same bits from call
 *      to call. */
int ddk_rconv_forward(ddk_ctx* ctx, int32_t layer, const float* x_nodes, int64_t n_in, int64_t n_out, const int32_t* edge_src, const int32_t* edge_dst,
                      const int32_t* src_order, const int64_t* src_ptr, const float* sh, const float* h, const int64_t* group_offsets, int32_t n_groups,
                      const float* w2, const float* b2, int64_t E, float* out_nodes, void* workspace, void* stream);

/* VJP of ddk_rconv_forward.  The same operands, and dst_order int32 [E] / dst_ptr int64 [n_in + 1] (the edge ids sorted by edge_dst in the same way),
 * grad_out_nodes [n_out, Dout].  grad_x_nodes [n_in, Din], grad_sh [E, 4], grad_h [E, 72], grad_w2 [n_groups, W, 72], grad_b2 [n_groups, W]: each may be
 * NULL (not computed); all five NULL is DDK_ERR_INVALID.  w2 and b2 may be NULL exactly when ddk_rtp_backward allows it.
 * workspace: ddk_rconv_workspace(layer, E, n_groups, n_in, n_out, 1) bytes, always needed when E > 0.  It holds gn = grad_out_nodes / max(count, 1)
 * [n_out, Dout] (made once per call, so that the kernels gather plain rows of it), the per-edge rows of grad_x [E, Din] (added per node in ascending edge
 * id, no atomics) and the parameter images of ddk_rtp_backward_workspace.  Never stored: [E, W] or its gradient, x_nodes[edge_dst] [E, Din], the
 * gathered rows of grad_out [E, Dout].
 * E == 0: the grad_x_nodes, grad_w2 and grad_b2 asked for are written as zeros, no kernel of the tensor product is launched.  Outputs must not alias
 * inputs.  The same bits from call to call, on every device, and whichever subset of the outputs is asked for. */
int ddk_rconv_backward(ddk_ctx* ctx, int32_t layer, const float* x_nodes, int64_t n_in, int64_t n_out, const int32_t* edge_src, const int32_t* edge_dst,
                       const int32_t* src_order, const int64_t* src_ptr, const int32_t* dst_order, const int64_t* dst_ptr, const float* sh, const float* h,
                       const int64_t* group_offsets, int32_t n_groups, const float* w2, const float* b2, const float* grad_out_nodes, int64_t E,
                       float* grad_x_nodes, float* grad_sh, float* grad_h, float* grad_w2, float* grad_b2, void* workspace, void* stream);

/* Bytes of the workspace of ddk_rconv_forward (backward == 0) or ddk_rconv_backward (backward != 0): a function of its arguments alone, whichever outputs
 * are asked for; -1 for a layer outside 0..4, DDK_TP_NV4 + 0..4 and DDK_TP_AA + 0..4, n_groups outside 1..4, E < 0 or E >= 2^31, n_in or n_out outside 0 .. 2^31 - 1.  Host function, no context. */
int64_t ddk_rconv_workspace(int32_t layer, int64_t E, int32_t n_groups, int64_t n_in, int64_t n_out, int32_t backward);

/* ---- The radial MLP's hidden layer from the edge embedding and the node table: the cat of the reference's embed loop (models/score_model.py:227-230) and
 *      fc[g][0..3] of the conv layer (Linear 72 -> 72, Identity, ReLU, Dropout; models/tensor_layers.py:154) as one op, the row [E, 72] of the cat never stored.
 *      For edge e of group g:
 *        pre[e, :] = b1[g] + w1[g] . [ emb[e, 0:24] | xs[edge_src[e], 0:24] | xs[edge_dst[e], 0:24] ]
 *        h[e, c]   = keep(e, c) ? max(pre[e, c], 0) * s : 0          s = 1.0f / (1.0f - p) in fp32;  p == 0: s = 1, keep is true everywhere, nothing is drawn
 *      xs [n_nodes, 24] (the scalar part of the node table, its own contiguous tensor), emb [E, 24], w1 [n_groups, 72, 72] (fc[g][0].weight stacked: columns
 *      0:24 meet emb, 24:48 the src row, 48:72 the dst row), b1 [n_groups, 72], h [E, 72]: DEVICE pointers, fp32, contiguous, 16-byte aligned.  edge_src,
 *      edge_dst: int32 [E], both index xs.  group_offsets, n_groups, E: as ddk_rtp_forward (HOST array).  0 <= p < 1, anything else is DDK_ERR_INVALID.
 *      The index tables are TRUSTED, as in ddk_rconv_forward: they must come from a validated graph (Context.conv_graph in Python).
 *      Exact fp32 in a fixed order: pre[e, c] is one fmaf chain over the 72 columns in ascending order that starts from b1[g][c].
 *
 *      THE DROPOUT MASK is a layout contract like DDK_RNG_LAYOUT: for a given DDK_RHID_MASK_LAYOUT it never changes.  keep(e, c) is a pure function of
 *      (seed, edge id e, column c); it does not depend on the launch grid, the device, the group table or the call.
 *        generator  Philox4x32-10 of csrc/k_philox.h (the sampler's)
 *        key        (seed_lo, seed_hi), the low and high words of `seed`
 *        counter    c0 = e_lo, c1 = e_hi (the 64-bit edge id), c2 = c / 4, c3 = DDK_RHID_MASK_TAG
 *        word       c % 4 of the block's four words
 *        rule       keep iff u >= p with u = (word >> 8) * 2^-24, the generator's uniform in [0, 1), compared in fp32
 *      No allocation, no synchronisation.  E == 0: DDK_OK, no launch. */
#define DDK_RHID_MASK_LAYOUT 1
#define DDK_RHID_MASK_TAG 0x52484944u      /* "RHID" */
int ddk_rhid_forward(ddk_ctx* ctx, const float* xs, int64_t n_nodes, const int32_t* edge_src, const int32_t* edge_dst, const float* emb,
                     const int64_t* group_offsets, int32_t n_groups, const float* w1, const float* b1, float p, uint64_t seed, int64_t E, float* h,
                     void* stream);

/* VJP of ddk_rhid_forward.  h: the forward's output, which carries the pattern of ReLU and Dropout: gpre[e, c] = grad_h[e, c] * (h[e, c] != 0 ? s : 0), so
 * the backward takes neither the seed nor a mask.  src_order / src_ptr, dst_order / dst_ptr: the node-sorted edge lists of ddk_rconv_backward over
 * edge_src and edge_dst, both with n_nodes + 1 pointer entries.  grad_xs [n_nodes, 24], grad_emb [E, 24], grad_w1 [n_groups, 72, 72], grad_b1 [n_groups, 72]:
 * each may be NULL (not computed); all four NULL is DDK_ERR_INVALID.  w1 may be NULL iff grad_xs == grad_emb == NULL.  b1 is not read.
 *   gin[e, :] = gpre[e, :] . w1[g]: columns 0:24 are grad_emb[e]; grad_xs[n] = (the sum of columns 24:48 over the edges with edge_src == n, in ascending edge
 *   id) + (the sum of columns 48:72 over the edges with edge_dst == n, in ascending edge id): a node without edges gets exact zeros.
 *   grad_w1[g] = sum_e gpre[e]^T (x) in[e], grad_b1[g] = sum_e gpre[e]: per slice of rtp-slice-length edges (a function of E alone) a partial image, the
 *   images added in slice order; a group without edges gets zeros.
 * workspace: ddk_rhid_workspace(E, n_groups, n_nodes) bytes of device memory, needed when E > 0, 16-byte aligned.  Its content, in this order, every part
 * padded to a multiple of four floats: the per-edge rows gin[:, 24:48] [E, 24]; the per-edge rows gin[:, 48:72] [E, 24]; the dst sum per node
 * [n_nodes, 24]; the parameter images [E / slice length + n_groups][72][73] (column 72 is grad_b1's).
 * E == 0: the grad_xs, grad_w1 and grad_b1 asked for are written as zeros, no kernel is launched.  Outputs must not alias inputs.  No atomics: the same bits
 * from call to call, on every device, and whichever subset of the outputs is asked for. */
int ddk_rhid_backward(ddk_ctx* ctx, const float* xs, int64_t n_nodes, const int32_t* edge_src, const int32_t* edge_dst, const int32_t* src_order,
                      const int64_t* src_ptr, const int32_t* dst_order, const int64_t* dst_ptr, const float* emb, const float* h,
                      const int64_t* group_offsets, int32_t n_groups, const float* w1, const float* grad_h, float p, int64_t E, float* grad_xs,
                      float* grad_emb, float* grad_w1, float* grad_b1, void* workspace, void* stream);

/* Bytes of ddk_rhid_backward's workspace: a function of its arguments alone; -1 for n_groups outside 1..4, E < 0 or E >= 2^31, n_nodes outside
 * 0 .. 2^31 - 1.  Host function, no context. */
int64_t ddk_rhid_workspace(int64_t E, int32_t n_groups, int64_t n_nodes);

/* ---- The head convolutions of the score model, node features to receiver rows: lines 153-159 of TensorProductConvLayer.forward (models/tensor_layers.py) for
 *      final_conv (head DDK_HEAD_CENTER) and tor_bond_conv (head DDK_HEAD_TORSION), both faster=False (e3nn's FullyConnectedTensorProduct), edge_groups=1,
 *      reduce='mean':
 *        out_nodes[r] = (sum over the edges e with edge_src[e] == r, in ascending e, of TP_head(x_nodes[edge_dst[e]], sh[e], w2 h[e] + b2)) / max(count, 1)
 *      x_nodes [n_in, 84] = [24x0e | 6x1o | 6x1e | 24x0o] (the output irreps of conv layer 3); sh [E, 4]; h [E, K] the radial MLP's hidden activation;
 *      w2 [W, K], b2 [W] its last Linear, in e3nn's instruction order.
 *        centre:  sh = (1x0e, 1x1o) of the edge, W = 144, K = 48, out_nodes [n_out, 12] = [2x1o | 2x1e].
 *        torsion: sh[e, 1:4] = the 1o block of FullTensorProduct(sh(edge), sh_2e(bond axis)) (sh[e, 0] is not read), W = 288, K = 72,
 *                 out_nodes [n_out, 48] = [24x0o | 24x0e].
 *      The graph tables are those of ddk_rconv_forward, and TRUSTED in the same way.  DEVICE pointers, fp32, contiguous; sh, h and the workspace 16-byte
 *      aligned.  workspace: ddk_hconv_workspace(head, E, n_in, n_out, 0) bytes: the [E, Dout] rows of the tensor product.  Never stored: the per-edge weights
 *      [E, W], the gathered rows [E, 84].  E == 0: out_nodes is written as zeros, no kernel is launched.  A receiver without edges: exact zeros.  No
 *      allocation, no synchronisation, no atomics: the same bits from call to call. */
#define DDK_HEAD_CENTER 0
#define DDK_HEAD_TORSION 1
int ddk_hconv_forward(ddk_ctx* ctx, int32_t head, const float* x_nodes, int64_t n_in, int64_t n_out, const int32_t* edge_src, const int32_t* edge_dst,
                      const int32_t* src_order, const int64_t* src_ptr, const float* sh, const float* h, const float* w2, const float* b2, int64_t E,
                      float* out_nodes, void* workspace, void* stream);

/* VJP of ddk_hconv_forward.  The same operands, dst_order / dst_ptr as ddk_rconv_backward, grad_out_nodes [n_out, Dout].  grad_x_nodes [n_in, 84],
 * grad_h [E, K], grad_w2 [W, K], grad_b2 [W]: each may be NULL (not computed); all four NULL is DDK_ERR_INVALID.  There is no grad_sh.  w2 may be NULL iff
 * grad_x_nodes == grad_h == NULL; b2 is read for grad_x_nodes alone.  workspace: ddk_hconv_workspace(head, E, n_in, n_out, 1) bytes, needed when E > 0: the
 * per-edge rows of grad_x [E, 84] (added per node in ascending edge id) and the parameter images [E / slice length + 1][W][K + 1] (one per slice of
 * rtp-slice-length edges, a function of E alone, added in slice order).  E == 0: the grad_x_nodes, grad_w2 and grad_b2 asked for are written as zeros.  A node
 * no edge reads: an exact zero row of grad_x_nodes.  Outputs must not alias inputs.  No atomics: the same bits from call to call, on every device, and
 * whichever subset of the outputs is asked for. */
int ddk_hconv_backward(ddk_ctx* ctx, int32_t head, const float* x_nodes, int64_t n_in, int64_t n_out, const int32_t* edge_src, const int32_t* edge_dst,
                       const int32_t* src_order, const int64_t* src_ptr, const int32_t* dst_order, const int64_t* dst_ptr, const float* sh, const float* h,
                       const float* w2, const float* b2, const float* grad_out_nodes, int64_t E, float* grad_x_nodes, float* grad_h, float* grad_w2,
                       float* grad_b2, void* workspace, void* stream);

/* Bytes of the workspace of ddk_hconv_forward (backward == 0) or ddk_hconv_backward (backward != 0): a function of its arguments alone; -1 for a head other
 * than the two above, E < 0 or E >= 2^31, n_in or n_out outside 0 .. 2^31 - 1.  Host function, no context. */
int64_t ddk_hconv_workspace(int32_t head, int64_t E, int64_t n_in, int64_t n_out, int32_t backward);

/* ---- The edge embeddings in front of the conv stack (models/score_model.py:191-225: lig_edge_embedding, cross_edge_embedding, rec_edge_embedding, each
 *      Linear(K, 24), ReLU, Dropout, Linear(24, 24)) with the edge's first-order spherical harmonics, ONE EDGE GROUP per call, as one op that stores nothing
 *      per edge besides its two outputs.  For edge e:
 *        vec       = pos_b[idx_b[e]] - pos_a[idx_a[e]],  d = |vec|
 *        row       = [ feat[e, 0:F] | sig[sig_index[idx_a[e]], 0:32] | exp(coeff (d - offset_j)^2), j = 0..31 ]            K = F + 64, F = 0 or 4
 *        hid[e, c] = keep(e, c) ? max(b1[c] + w1[c, :] . row, 0) * s : 0        s = 1.0f / (1.0f - p) in fp32;  p == 0: s = 1, nothing is drawn
 *        emb[e, :] = b2 + w2 . hid[e, :]                                        sh[e, :] = [1 | sqrt(3) vec / max(d, 1e-12)]
 *      offset = torch.linspace(start, stop, 32) in fp32 (step = (stop - start) / 31; offset_j = fmaf(step, j, start) for j < 16, fmaf(-step, 31 - j, stop) above) and
 *      coeff = -0.5 / (offset_1 - offset_0)^2, as GaussianSmearing (models/tensor_layers.py:171-181) states them; n_gauss must be 32.
 *      pos_a [n_a, 3], pos_b [n_b, 3], feat [E, 4] (NULL with F == 0; F is 0 or 4), sig [n_sig, 32] (the sigma embedding of every graph), w1 [24, K], b1 [24],
 *      w2 [24, 24], b2 [24], emb [E, 24], sh [E, 4]: DEVICE pointers, fp32, contiguous; feat, sig, emb and sh 16-byte aligned.  idx_a, idx_b: int32 [E];
 *      sig_index: int32 [n_a], the graph of node a.  The index tables are TRUSTED, as the graph tables of ddk_rconv_forward are.  0 <= p < 1.
 *      Exact fp32 in a fixed order: the pre-activation is one fmaf chain over the K columns in ascending order that starts from b1[c], emb[e, o] one fmaf
 *      chain over the 24 hidden columns in ascending order that starts from b2[o].
 *
 *      THE DROPOUT MASK is a layout contract like DDK_RHID_MASK_LAYOUT: for a given DDK_EEMB_MASK_LAYOUT it never changes.  keep(e, c) is a pure function of
 *      (seed, e, c), e the edge's position within the call (callers give every edge group a seed of its own):
 *        generator  Philox4x32-10 of csrc/k_philox.h;  key (seed_lo, seed_hi);  counter c0 = e_lo, c1 = e_hi, c2 = c / 4, c3 = DDK_EEMB_MASK_TAG
 *        word       c % 4 of the block's four words;  keep iff u >= p with u = (word >> 8) * 2^-24, compared in fp32
 *      No allocation, no synchronisation.  E == 0: DDK_OK, no launch. */
#define DDK_EEMB_MASK_LAYOUT 1
#define DDK_EEMB_MASK_TAG 0x45454D42u      /* "EEMB" */
int ddk_eemb_forward(ddk_ctx* ctx, const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, const int32_t* idx_a, const int32_t* idx_b,
                     const float* feat, int32_t F, const float* sig, int64_t n_sig, const int32_t* sig_index, float start, float stop, int32_t n_gauss,
                     const float* w1, const float* b1, const float* w2, const float* b2, float p, uint64_t seed, int64_t E, float* emb, float* sh,
                     void* stream);

/* VJP of ddk_eemb_forward for its parameters: the forward's operands (b2 is not read and may be NULL) and grad_emb [E, 24] (16-byte aligned).  There is no
 * input gradient: positions, times and bond types carry none in score matching.  The forward saves nothing per edge; row, the pre-activation and the mask
 * are recomputed here from the coordinates and the seed, with the forward's expressions.  grad_w1 [24, K], grad_b1 [24], grad_w2 [24, 24], grad_b2 [24]:
 * each may be NULL (not computed); all four NULL is DDK_ERR_INVALID.
 *   ghid[e, c] = fmaf chain over o ascending of grad_emb[e, o] w2[o, c], from 0;  gpre[e, c] = ghid[e, c] * (hid[e, c] != 0 ? s : 0)
 *   grad_w2 = sum_e grad_emb[e]^T (x) hid[e],  grad_b2 = sum_e grad_emb[e],  grad_w1 = sum_e gpre[e]^T (x) row[e],  grad_b1 = sum_e gpre[e]: per slice of
 *   rtp-slice-length edges (a function of E alone) a partial image, an fmaf chain over the slice's edges in ascending order, the images added in slice order.
 * workspace: ddk_eemb_workspace(E, K) bytes of device memory, needed when E > 0: the images [E / slice length + 1][24 (K + 1) + 24 25] and nothing else;
 * never an [E, .] tensor.  E == 0: the gradients asked for are written as zeros, no kernel is launched.  Outputs must not alias inputs.  No atomics: the
 * same bits from call to call, on every device, and whichever subset of the outputs is asked for. */
int ddk_eemb_backward(ddk_ctx* ctx, const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, const int32_t* idx_a, const int32_t* idx_b,
                      const float* feat, int32_t F, const float* sig, int64_t n_sig, const int32_t* sig_index, float start, float stop, int32_t n_gauss,
                      const float* w1, const float* b1, const float* w2, const float* b2, float p, uint64_t seed, const float* grad_emb, int64_t E,
                      float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2, void* workspace, void* stream);

/* Bytes of ddk_eemb_backward's workspace: a function of its arguments alone; -1 for K other than 64 and 68, E < 0 or E >= 2^31.  Host function, no context. */
int64_t ddk_eemb_workspace(int64_t E, int32_t K);

/* ---- The edge embeddings of the latent-conditioned (DisCo) score model, latent_dim = L in 1..4, latent_vocab = 1 (models/score_model.py:352-408 of the
 *      reference): ddk_eemb_forward with 2 L more columns behind the smearing and the unconditional embedding added to the output.  With ia = idx_a[e],
 *      ib = idx_b[e]:
 *        row       = [ feat[e] | sig[sig_index[ia]] | smearing(d) | lat_a[ia, 0:L] | lat_b[ib, 0:L] ]                K = F + 64 + 2 L;  w1 [24, K]
 *        hid, emb  as ddk_eemb_forward: the pre-activation's fmaf chain runs on over the 2 L new columns in ascending order; the mask is DDK_EEMB_MASK_LAYOUT's
 *        emb[e, o] = fmaf(unc_a[ia], uemb[o], emb[e, o])                                                             only where unc_a != NULL
 *      lat_a [n_a, L], lat_b [n_b, L]: node tables (they may be one table), unc_a [n_a]: the node's `unconditional` value (any float), uemb [24]: DEVICE,
 *      fp32, contiguous, the two tables 16-byte aligned.  zero_latent != 0 (the cross group): the row holds zeros in the 2 L columns, lat_a and lat_b are not
 *      read and may be NULL.  unc_a != NULL needs uemb.  Everything else as ddk_eemb_forward; with all-zero latents and no unconditional term emb has the
 *      bits of ddk_eemb_forward with w1[:, 0:K - 2 L] (fmaf(w, 0, acc) == acc for finite w). */
int ddk_eemb_latent_forward(ddk_ctx* ctx, const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, const int32_t* idx_a, const int32_t* idx_b,
                            const float* feat, int32_t F, const float* sig, int64_t n_sig, const int32_t* sig_index, float start, float stop, int32_t n_gauss,
                            const float* w1, const float* b1, const float* w2, const float* b2, float p, uint64_t seed, const float* lat_a, const float* lat_b,
                            int32_t L, int32_t zero_latent, const float* unc_a, const float* uemb, int64_t E, float* emb, float* sh, void* stream);

/* VJP of ddk_eemb_latent_forward: the four parameter gradients of ddk_eemb_backward (grad_w1 [24, K] with the 2 L latent columns; exact zeros there with
 * zero_latent), and because the latent DOES carry a gradient (the straight-through Gumbel softmax in front of it):
 *   grad_uemb [24]      = sum_e unc_a[ia] grad_emb[e, :], one more column of the slice images: an fmaf chain over the slice's edges in ascending order, the
 *                         images added in slice order; zeros where unc_a == NULL
 *   glat[e, j]          = fmaf chain over c ascending, from 0, of gpre[e, c] w1[c, F + 64 + j], j < 2 L: per-edge rows in the workspace, two planes [E, L]
 *   grad_lat_a [n_a, L] = the rows glat[e, 0:L] of the edges with idx_a[e] == n, added in ascending e (the first row starts the sum); grad_lat_b [n_b, L] the
 *                         same over glat[e, L:2 L] and idx_b.  order_a / ptr_a and order_b / ptr_b: the node-sorted edge lists of idx_a and idx_b (int32 [E],
 *                         int64 [n + 1], as ddk_seg_sum takes them; TRUSTED; needed only for the side whose gradient is asked for).  A node without edges
 *                         gets 0; with zero_latent both get zeros.  Where lat_a and lat_b are one table its gradient is grad_lat_a + grad_lat_b.
 * Each of the seven outputs may be NULL (not computed); all NULL is DDK_ERR_INVALID.  Everything is recomputed from the coordinates and the seed; the bits do
 * not depend on the subset asked for.  workspace: ddk_eemb_latent_workspace(E, K, L) bytes, needed when E > 0: the images, the [E, 2 L] rows, nothing wider.
 * E == 0: the outputs asked for are written as zeros, no kernel is launched.  No atomics. */
int ddk_eemb_latent_backward(ddk_ctx* ctx, const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, const int32_t* idx_a, const int32_t* idx_b,
                             const float* feat, int32_t F, const float* sig, int64_t n_sig, const int32_t* sig_index, float start, float stop, int32_t n_gauss,
                             const float* w1, const float* b1, const float* w2, const float* b2, float p, uint64_t seed, const float* lat_a, const float* lat_b,
                             int32_t L, int32_t zero_latent, const float* unc_a, const float* uemb, const int32_t* order_a, const int64_t* ptr_a,
                             const int32_t* order_b, const int64_t* ptr_b, const float* grad_emb, int64_t E, float* grad_w1, float* grad_b1, float* grad_w2,
                             float* grad_b2, float* grad_uemb, float* grad_lat_a, float* grad_lat_b, void* workspace, void* stream);

/* Bytes of ddk_eemb_latent_backward's workspace; -1 for L outside 1..4, K other than 64 + 2 L and 68 + 2 L, E < 0 or E >= 2^31.  Host function, no context. */
int64_t ddk_eemb_latent_workspace(int64_t E, int32_t K, int32_t L);

/* ---- The ragged straight-through Gumbel softmax that makes the latent of a collated batch (latent_encoder.py:328-335 and pretrained_score_encoder.py:74-81
 *      of the reference, over models/layers.py:152-181): per graph g and latent dimension d, over the graph's ligand nodes followed by its receptor nodes
 *      (position pos = 0 .. n_g - 1):
 *        gum = -log(-log(u + 1e-20f) + 1e-20)     z = (logit + gum) / T     e = exp(z - max z)  in fp64 (u + 1e-20f in fp32), e rounded to fp32 once: z is
 *        1 / T times a number of the order of 10, and an fp32 z would hand its ulp (6e-5 at T = 0.01) to every y as a relative error;
 *        y = e / sum     out = (hard - y) + y  in fp32, hard = 1 at the LOWEST position of the maximum of y, else 0.  The sum of the softmax in a fixed order: thread t of 256 adds the positions of the quads
 *        t, t + 256, ... (four positions each) in ascending order from 0, the partials by a halving tree.
 *      logit_l / y_l / out_l [n_lig, D], logit_r / y_r / out_r [n_rec, D]: DEVICE, fp32, contiguous; lig_ptr, rec_ptr: DEVICE int64 [G + 1], graph g owns the
 *      rows ptr[g] .. ptr[g + 1] - 1 (a pair that is no range of its table: the graph is left unwritten); stream_id: DEVICE uint64 [G].  y is saved for the
 *      backward:  grad_logit = y * (grad_out - sum grad_out y) / T  with the sum in the same order.  One launch each, one workgroup per (g, d), no atomics.
 *      THE NOISE is a layout contract: for a given DDK_GUMBEL_LAYOUT it never changes.  Generator purpose 13 of DDK_RNG_LAYOUT 1 with counter (stream_id[g],
 *      sample, 13 << 28 | draw << 8 | d) yields four words; words 0 and 1 are the KEY of a second Philox4x32-10 whose counter (pos / 4, 0, 0, DDK_GUMBEL_TAG)
 *      gives position pos the word pos % 4; u = (word >> 8) * 2^-24.  A graph's noise is a pure function of (seed, complex, sample, draw, d, pos), whatever
 *      the batch; no existing purpose is touched; no node limit.  Limits: 1 <= G <= 65536, 1 <= D <= 4, 0 <= draw < 2^20, sample >= 0, T > 0 and finite.
 *
 *      ddk_gumbel_pick_samples: the one-hot latents of B samples of ONE complex from ONE table of logits (the oracle encoder in front of the sampler reads only
 *      the true pose, so its logits are the same for every copy of the complex in a batch).  Rows b n .. (b + 1) n - 1 of lig_latent [B n_lig, D] and rec_latent
 *      [B n_rec, D] are, BIT FOR BIT, out_l and out_r of ddk_gumbel_softmax_batch called with G = 1, stream id ``stream_id``, sample = sample0 + b and the same
 *      seed, draw and T (one device body serves both kernels): the noise is the same DDK_GUMBEL_LAYOUT, no new number.  choices (DEVICE int32 [B, D], or NULL):
 *      the position of the one, ligand nodes first, then n_lig + the receptor index (the convention of ddk_ar_decode); -1 where no y compares (NaN logits).
 *      One launch, one workgroup of 256 threads per (b, d), no atomics; the soft y lives in a grow-only scratch buffer of the context (B (n_lig + n_rec) D
 *      floats).  stream_id is passed by value.  Limits: 1 <= B <= 65536, 1 <= D <= 4, T > 0 and finite, 0 <= draw < 2^20, sample0 >= 0 and
 *      sample0 + B - 1 < 2^31, n_lig + n_rec < 2^31; a violation or a null pointer of a side that has nodes is DDK_ERR_INVALID before any launch, and the
 *      outputs stay untouched.  n_lig + n_rec == 0 writes nothing.
 *
 *      ddk_rng_latent_keep: the per-complex keep flag of the latent dropout (classifier-free guidance training), keep_out[i] = (u >= rate) as 1.0f / 0.0f with u
 *      the uniform of purpose 12 for (seed, stream_id[i], sample, draw), block 0, word 0.  A HOST function as ddk_rng_forward_times. */
#define DDK_GUMBEL_LAYOUT 1
#define DDK_GUMBEL_TAG 0x47554D42u      /* "GUMB" */
int ddk_gumbel_softmax_batch(ddk_ctx* ctx, int32_t G, int32_t D, const float* logit_l, int64_t n_lig, const float* logit_r, int64_t n_rec,
                             const int64_t* lig_ptr, const int64_t* rec_ptr, float T, uint64_t seed, const uint64_t* stream_id /* DEVICE [G] */, int32_t sample,
                             int32_t draw, float* y_l, float* y_r, float* out_l, float* out_r, void* stream);
int ddk_gumbel_softmax_batch_backward(ddk_ctx* ctx, int32_t G, int32_t D, const float* y_l, int64_t n_lig, const float* y_r, int64_t n_rec,
                                      const int64_t* lig_ptr, const int64_t* rec_ptr, float T, const float* grad_out_l, const float* grad_out_r,
                                      float* grad_logit_l, float* grad_logit_r, void* stream);
int ddk_gumbel_pick_samples(ddk_ctx* ctx, int32_t B, int32_t D, const float* logit_l /* [n_lig, D] */, int64_t n_lig, const float* logit_r /* [n_rec, D] */,
                            int64_t n_rec, float T, uint64_t seed, uint64_t stream_id, int32_t sample0, int32_t draw, float* lig_latent /* [B*n_lig, D] */,
                            float* rec_latent /* [B*n_rec, D] */, int32_t* choices /* [B, D] or NULL */, void* stream);
int ddk_rng_latent_keep(ddk_ctx* ctx, uint64_t seed, int32_t n, const uint64_t* stream_id /* HOST [n] */, int32_t sample, int32_t draw, float rate,
                        float* keep_out /* HOST [n] */);

/* ---- The AR latent model's loss: cross-entropy over a graph's ligand nodes followed by its receptor nodes (position p = 0 .. n_g - 1), the reference's loop
 *      of one F.cross_entropy per graph (autoregressive/train_ar.py:116-127, 152-177) for a collated batch in one launch, one workgroup of 256 threads per
 *      graph.  s_p: the student's logit, logit_l [n_lig] / logit_r [n_rec] (the AR predictors emit one column); t_p: column c = column[g] of the teacher's
 *      tables teacher_l [n_lig, D] / teacher_r [n_rec, D], 1 <= D <= 4.  The arithmetic, every reduction in fp64 and every operation as written:
 *        pick   = the LOWEST p that holds max s_p        target = the LOWEST p that holds max t_p     (no p above -inf: position 0)
 *        lse_s  = m_s + log(sum exp(s_p - m_s)), m_s = max s_p.  The sum in a fixed order: thread t of 256 adds the positions of the quads t, t + 256, ...
 *                 (four positions each) in ascending order to a partial that starts from 0, the partials are added by a halving tree
 *        soft = 0 (the reference's sampled labels):  q = target, loss = fl32(lse_s - s_q)
 *        soft = 1 (its --no_sampling: the label is softmax of the encoder's logits):  lse_t as lse_s, p_t = exp(t_p - lse_t),
 *                 loss = fl32(lse_s - sum p_t s_p), summed in the same order
 *      out, [G] each: loss (fp32), pick, target (int64), and saved [G, 2] = (lse_s, lse_t) in fp64, which with target is all the backward needs: nothing
 *      is saved per node.  The backward takes grad [G] and writes, element-wise in fp32,
 *        grad_logit_p = grad_g * (fl32(exp(s_p - lse_s)) - target_p),   target_p = [p == q] (soft = 0) or fl32(exp(t_p - lse_t)) (soft = 1)
 *      for EVERY row of a graph with valid tables, rows whose gradient is zero included; with soft = 0 it reads no teacher table (they may be NULL).
 *      lig_ptr / rec_ptr: DEVICE int64 [G + 1], graph g owns the rows ptr[g] .. ptr[g + 1] - 1; column: DEVICE int32 [G].  A graph whose pointer pair is no
 *      range of its table, whose column is outside 0 .. D - 1, or that has no node is left alone: none of its outputs is written, in either direction.
 *      All tables DEVICE, fp32, contiguous.  One launch each, no atomics, no scratch, no node limit.  Limits: 1 <= G <= 65536, 1 <= D <= 4, soft 0 or 1. */
int ddk_node_cross_entropy_batch(ddk_ctx* ctx, int32_t G, int32_t D, const float* logit_l, int64_t n_lig, const float* logit_r, int64_t n_rec,
                                 const int64_t* lig_ptr, const int64_t* rec_ptr, const float* teacher_l, const float* teacher_r, const int32_t* column,
                                 int32_t soft, float* loss, int64_t* pick, int64_t* target, double* saved /* [G, 2] */, void* stream);
int ddk_node_cross_entropy_batch_backward(ddk_ctx* ctx, int32_t G, int32_t D, const float* logit_l, int64_t n_lig, const float* logit_r, int64_t n_rec,
                                          const int64_t* lig_ptr, const int64_t* rec_ptr, const float* teacher_l, const float* teacher_r,
                                          const int32_t* column, int32_t soft, const float* grad /* [G] */, const int64_t* target, const double* saved,
                                          float* grad_logit_l, float* grad_logit_r, void* stream);
/* ddk_rng_decoding_index: the decoding index of an AR training item (autoregressive/dataset_ar.py:83 draws it from an unseeded host generator),
 * idx_out[i] = ((word >> 8) * D) >> 24 in integer arithmetic, in 0 .. D - 1, with `word` word 0 of block 0 of purpose 14 for (seed, stream_id[i], sample, draw).
 * A HOST function as ddk_rng_latent_keep; 1 <= D <= 4. */
int ddk_rng_decoding_index(ddk_ctx* ctx, uint64_t seed, int32_t n, const uint64_t* stream_id /* HOST [n] */, int32_t sample, int32_t draw, int32_t D,
                           int32_t* idx_out /* HOST [n] */);

/* The fixed-order segmented sum the radial conv and the head convs add a node's rows with (rtp_seg_kernel of csrc/k_rtp.hip), on its own: the backward of
 * a gather x[index].  nodes[n, :] = rows[order[ptr[n]], :] + rows[order[ptr[n] + 1], :] + ... + rows[order[ptr[n + 1] - 1], :], added in that order, one
 * thread per (node, column); a node without rows: exact zeros.  rows [*, D], nodes [n_nodes, D]: DEVICE, fp32, contiguous, 1 <= D <= 128; order: int32,
 * ptr: int64 [n_nodes + 1], TRUSTED as the graph tables of ddk_rconv_forward (Context.conv_graph makes them).  n_nodes == 0: DDK_OK, no launch.  No
 * allocation, no synchronisation, no atomics: the same bits from call to call. */
int ddk_seg_sum(ddk_ctx* ctx, const float* rows, const int32_t* order, const int64_t* ptr, float* nodes, int64_t n_nodes, int32_t D, void* stream);

/* ---- a11: TensorProductConvLayer.forward(node_attr, edge_index, edge_attr, edge_sh)
 *      models/tensor_layers.py:147-168 for conv layer `layer`, fused: radial MLP (fp32 MFMA) +
 *      tensor product + segmented scatter-sum + mean + BatchNorm(eval) + residual, without ever
 *      materialising the [E, W] weight tensor.
 *      x [N, Din]; edge_src/edge_dst [E] int32 (edge_index rows 0/1); group_offsets[5] HOST array
 *      (edge ranges of the 4 edge groups, group g uses fc[g]); edge_attr [E, 3*ns] (the
 *      concatenated per-group edge_attr list); sh [E,4]; out [N, Dout]. */
int ddk_conv_forward(ddk_ctx* ctx, int32_t layer, const float* x, int64_t N, const int32_t* edge_src,
                     const int32_t* edge_dst, const int64_t* group_offsets, const float* edge_attr,
                     const float* sh, float* out, void* stream);

/* ---- one complex: the graph tensors datasets_utils/process_mols.py emits.
 *      All pointers are HOST pointers; the library uploads them and precomputes everything that is
 *      constant over the reverse-diffusion steps and over the samples (receptor embedding without
 *      its sigma part, receptor-receptor geometry). */
typedef struct ddk_complex_desc {
  int32_t n_lig, n_rec, n_bond_edges /* directed, = 2*bonds */, n_rot, n_rec_edges, rec_feat_dim /* 1 + lm dim */;
  const int32_t* lig_x;          /* [n_lig, 16]   data['ligand'].x */
  const int32_t* bond_index;     /* [2, n_bond_edges]   data['ligand','ligand'].edge_index */
  const float* bond_attr;        /* [n_bond_edges, 4]   .edge_attr */
  const uint8_t* edge_mask;      /* [n_bond_edges]      data['ligand'].edge_mask */
  const uint8_t* mask_rotate;    /* [n_rot, n_lig]      data['ligand'].mask_rotate */
  const float* rec_x;            /* [n_rec, rec_feat_dim] data['receptor'].x */
  const float* rec_pos;          /* [n_rec, 3] */
  const int32_t* rec_edge_index; /* [2, n_rec_edges]    data['receptor','receptor'].edge_index */
} ddk_complex_desc;

int ddk_complex_create(ddk_ctx* ctx, const ddk_complex_desc* desc, int32_t max_batch, ddk_complex** out);
void ddk_complex_destroy(ddk_ctx* ctx, ddk_complex* cx);

/* ---- all-atom confidence model (models/all_atom_score_model.py in confidence_mode; context created with all_atoms = 1 and
 *      the reference's confidence checkpoint keys): the receptor-atom level of the graph (datasets_utils/process_mols.py:383-477),
 *      HOST pointers; ddk_complex_set_atoms also needs the complex's ligand ids and receptor features again because the node
 *      embeddings of this model (OldAtomEncoder, models/layers.py:81-116) are computed here. */
typedef struct ddk_atoms_desc {
  int32_t n_atom, n_atom_edges;
  const int32_t* atom_x;          /* [n_atom, 4]   data['atom'].x */
  const float* atom_pos;          /* [n_atom, 3] */
  const int32_t* atom_edge_index; /* [2, n_atom_edges]  data['atom','atom'].edge_index */
  const int32_t* atom_rec_index;  /* [2, n_atom]        data['atom','receptor'].edge_index (row 0 = arange) */
} ddk_atoms_desc;
int ddk_complex_set_atoms(ddk_ctx* ctx, ddk_complex* cx, const ddk_atoms_desc* atoms, const int32_t* lig_x, const float* rec_x,
                          int32_t rec_feat_dim);

/* confidence_model(batch) -> [B, num_confidence_outputs]  (utils/sampling.py:230-243 with set_time(..., 0, 0, 0);
 * models/all_atom_score_model.py:203-284): lig_pos [B, n_lig, 3] DEVICE, out [B, num_confidence_outputs] DEVICE. */
int ddk_confidence_forward(ddk_ctx* ctx, ddk_complex* cx, int32_t B, const float* lig_pos, float* out, void* stream);

/* confidence_model(complex_graph_batch) of utils/sampling.py:239-240 - the branch WITHOUT confidence_data_list: a coarse-grained confidence
 * model (ddk_config.confidence_mode) evaluated on the score model's own graphs at the final poses.  The reference does not reset the times in that
 * branch: (t_tr, t_rot, t_tor) are the LAST step's schedule values, which confidence_mode uses as sigmas (models/score_model.py:186-189).
 * cx: a complex created in THIS context from the same ddk_complex_desc the score model's was; lig_pos [B, n_lig, 3] DEVICE,
 * out [B, num_confidence_outputs] DEVICE. */
int ddk_score_confidence(ddk_ctx* ctx, ddk_complex* cx, int32_t B, const float* lig_pos, float t_tr, float t_rot, float t_tor, float* out,
                         void* stream);

/* Status words of the last ddk_confidence_forward of `cx`, copied WITHOUT synchronising: enqueues an asynchronous copy of 20 int32 into
 * host_out (HOST, pinned memory if the copy is to overlap): [0..8] first edge and [9..17] end of the nine edge groups [ll lr la aa al ar
 * rr rl ra], [18] ligand-atom edge cursor, [19] != 0: the ligand-atom edge capacity overflowed (the confidences of that batch are invalid;
 * the Python shim raises).  Valid once the stream has passed the copy. */
int ddk_confidence_status(ddk_ctx* ctx, ddk_complex* cx, int32_t* host_out, void* stream);

/* ---- DisCo latent conditioning (models/score_model.py:170-184, 209-215, 329-337, 358-366, 392-402; latent_vocab == 1):
 *      lig_latent [B*n_lig, latent_dim], rec_latent [B*n_rec, latent_dim] (data['ligand'|'receptor'].latent_h, DEVICE,
 *      caller-owned, must stay valid for the following forwards) and the value of data[...].unconditional.
 *      Applies to the subsequent ddk_score_forward / ddk_sample calls on this complex; NULL, NULL clears.
 *      The library derives a per-sample edge group from WHERE the receptor latents are non-zero (layer-0 de-duplication)
 *      when the first forward after this call runs: call ddk_set_latents again after changing the arrays in place (ddk_ar_decode does
 *      this bookkeeping itself). */
int ddk_set_latents(ddk_ctx* ctx, ddk_complex* cx, const float* lig_latent, const float* rec_latent, float unconditional);

/* ---- a22: the AR latent model (config 3).  A context that was given the AR checkpoint (its own score-model copy under the plain
 *      key names + latent_s_predictor.* / latent_r_predictor.*) evaluates, after a forward at t = 1 with unconditional = 1, the
 *      partially decoded latents bound by ddk_set_latents and ddk_set_keep_receptor_features(on)  (= score_model.embed(),
 *      models/pretrained_score_encoder.py:58-75):
 *      ddk_ar_logits: the two predictor MLPs (Linear-BatchNorm1d-ReLU-Linear-BatchNorm1d-ReLU-Linear, :24-45) on the scalar
 *        channels [x[:, :ns] | x[:, -ns:]] of every node -> logits [B, n_lig + n_rec] (ligand atoms first, :84-88), DEVICE;
 *      ddk_ar_decode: GenericEncoder.encode_ar's pick for latent dimension decoding_idx (models/model_classes.py:21-47):
 *        logits * temperature; temperature >= 100: argmax; else index i with probability exp(.)_i / sum (NaN -> 0, inf -> FLT_MAX
 *        like torch.nan_to_num), drawn by inverse CDF from the caller's uniforms [B] in [0,1) (DEVICE; the reference calls
 *        torch.multinomial: same distribution, the draws stay with the caller); sets lig_latent[b*n_lig + c, decoding_idx] = 1 or
 *        rec_latent[b*n_rec + c - n_lig, decoding_idx] = 1 ([B*n, latent_dim] DEVICE arrays the caller zeroed) and, when not NULL,
 *        choices[b, decoding_idx] = c ([B, latent_dim] int32 DEVICE). */
int ddk_ar_logits(ddk_ctx* ctx, ddk_complex* cx, int32_t B, float* logits_out, void* stream);
int ddk_ar_decode(ddk_ctx* ctx, ddk_complex* cx, int32_t B, const float* logits, float temperature, const float* uniforms,
                  int32_t decoding_idx, int32_t latent_dim, float* lig_latent, float* rec_latent, int32_t* choices, void* stream);

/* ---- classifier-free guidance of the sampler (utils/sampling.py:119-135): while cfg_end <= t_tr <= cfg_start every step of
 *      ddk_sample runs a second forward with unconditional = 1 and zeroed latents and uses
 *      score + weight * (score - score_unconditional).  weight = 0 (default) disables it. */
int ddk_set_guidance(ddk_ctx* ctx, ddk_complex* cx, float weight, float cfg_start, float cfg_end);

/* ---- The heads read ligand rows only (models/score_model.py:286-308), so by default the LAST conv layer evaluates only
 *      the messages into ligand nodes (edge groups lig-lig and lig->rec) and the receptor rows after it are not produced.
 *      Turn this on before a forward whose receptor rows will be read with ddk_last_node_features (the embed() path of
 *      the AR latent model, models/pretrained_score_encoder.py:66-75): the last layer then evaluates all four groups as
 *      the reference does.  tr/rot/tor are identical either way. */
int ddk_set_keep_receptor_features(ddk_ctx* ctx, ddk_complex* cx, int32_t on);

/* ---- Backward receptive-field pruning (default ON; exact in real arithmetic): because the heads read ligand rows only, conv
 *      layer L-2 has to produce receptor rows only at the residues that carry a cross edge, layer L-3 only at those plus the
 *      senders of their receptor-receptor messages, and so on (csrc/k_graph.hip).  The receptor-receptor messages outside that
 *      set are not evaluated.  tr/rot/tor are unchanged (tests: test_pruned_layers_equal_full); 0 switches it off (every layer
 *      evaluates every receptor-receptor message, as the reference does).  Forwards with ddk_set_keep_receptor_features(on)
 *      never prune.  In a confidence-model context the same switch governs the level-A / level-B pruning of the static edge groups in its
 *      second- and third-to-last layers (the predictor pools ligand rows only; DESIGN.md 3.2, test_confidence_level_a_pruning_equal_full). */
int ddk_set_receptive_field_pruning(ddk_ctx* ctx, int32_t on);

/* ---- a5-a17: model.score_model(batch) -> (tr[B,3], rot[B,3], tor[B*R])  models/score_model.py:259-308
 *      for B copies of one complex at a common time (utils/sampling.py:113-117).
 *      lig_pos [B, n_lig, 3]; outputs tr [B,3], rot [B,3], tor [B*n_rot]. */
int ddk_score_forward(ddk_ctx* ctx, ddk_complex* cx, int32_t B, const float* lig_pos, float t_tr, float t_rot,
                      float t_tor, float* tr_out, float* rot_out, float* tor_out, void* stream);

/* ---- a18-a21: modify_conformer_batch(pos, data, tr_update, rot_update, torsion_updates, mask_rotate)
 *      utils/diffusion_utils.py:37-55 (axis-angle rotation, sequential torsion updates, Kabsch re-alignment).
 *      pos [B,n_lig,3], tr [B,3], rot [B,3], tor [B*n_rot] (may be NULL: rigid only) -> pos_out [B,n_lig,3]. */
int ddk_se3_update(ddk_ctx* ctx, ddk_complex* cx, int32_t B, const float* pos, const float* tr, const float* rot,
                   const float* tor, float* pos_out, void* stream);

/* ---- randomize_position(data_list, no_torsion, no_random, tr_sigma_max)  utils/sampling.py:12-34 for B copies of one
 *      complex in one launch: per sample  pos = torsions(pos0, tor[b])  (bond order, utils/torsion.py:48-68,
 *      zero updates skipped);  pos = (pos - mean(pos)) @ rot[b]^T + tr[b].
 *      pos0 [n_lig,3] the conformer (DEVICE); tor [B, n_rot] = np.random.uniform(-pi, pi) draws or NULL (no_torsion);
 *      rot [B,3,3] row-major rotation matrices (scipy Rotation.random().as_matrix()); tr [B,3] = N(0, tr_sigma_max) draws or
 *      NULL (no_random); pos_out [B,n_lig,3].  The draws stay with the caller: the reference's host RNG streams or device RNG. */
int ddk_randomize_position(ddk_ctx* ctx, ddk_complex* cx, int32_t B, const float* pos0, const float* tor, const float* rot,
                           const float* tr, float* pos_out, void* stream);

/* ---- pose metrics of evaluate.py:297-338 for B poses of one complex, one launch:
 *      out[b] = { rmsd, centroid_distance, min_cross_distance, min_self_distance } with
 *        rmsd = min over k < n_perms of sqrt(mean_i |pos[perms[k][i]] - ref[i]|^2)
 *               = the symmetry-corrected RMSD of evaluate.py:308-310 (spyrmsd.rmsd.symmrmsd, no minimisation: the minimum over the
 *               graph automorphisms of the ligand).  perms [n_perms, n_lig] int32 DEVICE: row k maps every ligand atom i to its image
 *               (computed once per ligand on the caller's side, INTEGRATION.md shows the spyrmsd / networkx recipe; row 0 should be
 *               the identity; entries of masked-out atoms are ignored; a row with an entry outside [0, n_lig) is checked on the device and
 *               never wins the minimum - rmsd = inf if no row is valid).  perms = NULL, n_perms = 0: identity only = the uncorrected
 *               fallback of evaluate.py:313.
 *        centroid_distance = |mean_i pos_i - mean_i ref_i|         (:315)
 *        min_cross_distance = min over receptor points r, atoms i of |rec_r - pos_i|   (:331-332): rec_atom_pos [n_rec_atoms, 3] DEVICE,
 *               the receptor ATOM coordinates the reference reads from the PDB file minus original_center; NULL, 0: the C-alpha
 *               coordinates of the complex
 *        min_self_distance  = min over atom pairs i != j of |pos_i - pos_j|          (:333-335)
 *      all over the atoms with atom_mask[i] != 0 (filterHs, evaluate.py:297).  pos [B,n_lig,3], ref_pos [n_lig,3] (already minus
 *      original_center), atom_mask [n_lig] uint8 (NULL = all atoms), out [B,4]; all DEVICE pointers. */
int ddk_pose_metrics(ddk_ctx* ctx, ddk_complex* cx, int32_t B, const float* pos, const float* ref_pos, const uint8_t* atom_mask,
                     const int32_t* perms, int32_t n_perms, const float* rec_atom_pos, int32_t n_rec_atoms, float* out, void* stream);

/* ---- poses in -> distinct binding modes out, without a ground truth: the all-pairs form of the RMSD above and a clustering on it.
 *      Neither call takes a ddk_complex: nothing of a complex is read, so poses from any source can be clustered.  Neither synchronises or allocates.
 *
 *      ddk_pose_pairwise_rmsd: pos [B, n_lig, 3] -> out [B, B] fp32 (all DEVICE), one launch:
 *        out[i][i] = 0;  for i < j:  out[i][j] = out[j][i] = min over k < n_perms of sqrt((1/m) sum over kept a of |pos_i[perms[k][a]] - pos_j[a]|^2)
 *      The lower-indexed pose is the permuted one: ddk_pose_metrics' convention with pose j as ref.  Only i < j is computed and the value is
 *      stored twice, so the matrix is symmetric bit for bit.  No alignment: the poses share the receptor frame (evaluate.py:313).
 *      atom_mask [n_lig] uint8 (NULL = all atoms), m = the number of kept atoms; m = 0 gives a matrix of zeros.  perms [n_perms, n_lig] int32 is
 *      ddk_pose_metrics' automorphism table (perms = NULL, n_perms = 0: identity only; entries of masked-out atoms are ignored; a row with a kept
 *      entry outside [0, n_lig) is detected on the device and never wins the minimum; if no row is valid the off-diagonal entries are +inf,
 *      never NaN).  Coordinate differences are taken first and then squared (exact 150 A from the origin where |a|^2 + |b|^2 - 2ab cancels),
 *      summed in fp32, one sqrt per pair after the minimum; no float atomics: bit-identical run to run.
 *      Limits: 1 <= n_lig <= 256, 1 <= B <= 4096; anything else is DDK_ERR_INVALID.
 *
 *      ddk_pose_cluster: greedy leader clustering on such a matrix rmsd [B, B], 1 <= B <= 1024 (one workgroup):
 *        rank the samples by score [B] descending (ties to the lower index; NaN ranks below -inf, NaNs among themselves by index;
 *        score = NULL: index order); walk the ranking: an unassigned sample becomes the next leader, and every unassigned sample c with
 *        rmsd[leader][c] <= cutoff joins it.  An entry equal to the cutoff joins; an inf (or NaN) entry never joins, under cutoff = inf too.
 *      Outputs, int32 DEVICE arrays: cluster [B] the cluster ordinal of each sample in discovery order (0 = the cluster of the top-scored
 *      pose); leaders [B] the leader's sample index of each cluster in its first n_clusters entries, -1 after them; n_clusters [1]. */
int ddk_pose_pairwise_rmsd(ddk_ctx* ctx, int32_t B, int32_t n_lig, const float* pos, const uint8_t* atom_mask,
                           const int32_t* perms, int32_t n_perms, float* out, void* stream);
int ddk_pose_cluster(ddk_ctx* ctx, int32_t B, const float* rmsd, const float* score, float cutoff,
                     int32_t* cluster, int32_t* leaders, int32_t* n_clusters, void* stream);

/* ---- the automorphism table the three calls above read, enumerated on the device: every colour- and bond-preserving bijection of the ligand's kept
 *      atoms.  The reference gets it from spyrmsd under time_limit(10) (utils/utils.py:84-98) and falls back to the uncorrected RMSD when that raises
 *      (evaluate.py:308-313), which is what happens to the ligands with the largest symmetry groups.  Like the two calls above this one takes no
 *      ddk_complex, allocates nothing and does not synchronise; all pointers are DEVICE pointers.
 *        colour [n_lig] int32: atoms may map to atoms of the same colour only (the element index, column 0 of lig_x).
 *        bond_index [2, n_bond_edges] int32: covalent bonds; duplicate columns and the two directions of a bond are one edge, a column with two equal
 *               ends is ignored.  NULL only with n_bond_edges = 0.
 *        atom_mask [n_lig] uint8 (NULL = all atoms): the kept atoms.  Masked-out atoms and their bonds are not part of the graph (remove_all_hs).
 *        perms_out [cap, n_lig] int32: row k maps a kept atom a to its image and a masked-out atom to itself: ddk_pose_metrics' table.  Row 0 is the
 *               identity.  The rows come in a fixed order (a breadth-first matching order, images ascending): bit-identical run to run.
 *        count_out [2] int32: [0] the rows written (>= 1), [1] the status: 0 complete; 1 overflow: some level of the search held more than cap
 *               partial maps (never fewer than the K automorphisms; cap = 2 K is enough for every graph in tests/automorphism_ref.py); 2 a bond index
 *               outside [0, n_lig), found on the device before it is used as an address.  With status 1 or 2 the identity is the only row (the
 *               uncorrected fallback, as in the reference) and nothing past it is written.  Overflow is a result, not an error: the call returns DDK_OK.
 *        workspace: ddk_ligand_automorphisms_workspace(n_lig, cap) bytes of device memory, 16-byte aligned, contents irrelevant before and after
 *               (about 2 * cap * n_lig bytes; a host function, no context; -1 if a limit is broken).
 *      The search is level-synchronous over partial maps (csrc/k_autos.hip): one workgroup walks the levels while they are small, larger levels take a
 *      pair of launches each over a fixed grid; the host enqueues 2 * n_lig launches without knowing the frontier sizes, which stay on the device.
 *      Limits: 1 <= n_lig <= 256, n_bond_edges >= 0, 1 <= cap <= 2^20; anything else is DDK_ERR_INVALID. */
int64_t ddk_ligand_automorphisms_workspace(int32_t n_lig, int32_t cap);
int ddk_ligand_automorphisms(ddk_ctx* ctx, int32_t n_lig, const int32_t* colour, const int32_t* bond_index, int32_t n_bond_edges,
                             const uint8_t* atom_mask, int32_t* perms_out, int32_t cap, int32_t* count_out /* [2] */,
                             void* workspace, void* stream);

/* ---- coordinates + bonds in -> the static graph tables ddk_complex_create and ddk_complex_set_atoms take, built on the device (csrc/k_build.hip) instead of
 *      by the host code of the reference's data pipeline (scipy cdist + a Python loop, torch_cluster, networkx).  Like ddk_ligand_automorphisms the three
 *      calls take no ddk_complex, allocate nothing and do not synchronise; all pointers are DEVICE pointers; the work is enqueued on `stream`; the caller
 *      owns a workspace of *_workspace(...) bytes (16-byte aligned, contents irrelevant before and after; a host function, no context, -1 if a limit is
 *      broken); count_out [2] int32 = {count, status}.  A status other than 0 is a result: the call returns DDK_OK.  A broken limit or a NULL argument is
 *      DDK_ERR_INVALID.  No float atomics and no atomic cursors: the order of the output is fixed and it is bit-identical run to run.
 *      Distances: the fp32 coordinates are converted to double, subtracted, d2 = dx*dx + dy*dy + dz*dz in double, compared with (double)r * (double)r,
 *      strictly below.  (On coordinates that are small multiples of 0.5 every step is exact, whatever the contraction.)
 *
 *      ddk_receptor_knn_graph: rec_edge_index by the rule of get_calpha_graph, datasets_utils/process_mols.py:337-353.  pos [n, 3].  Row i's candidates
 *        are the j != i with d(i, j) < cutoff.  At most max_neighbor of them: all are kept, in ascending j (np.where order).  More: the max_neighbor nearest
 *        of ALL other points, ordered by ascending (d2, j): nearest first, ties to the lower index.  None: the single nearest other point, ties to the
 *        lower index.  Self is excluded by its INDEX: a coincident residue j != i is a neighbour at distance 0 like any other, where the reference drops
 *        position 0 of the argsort and its `assert i not in dst` fires.  edge_index_out [2, cap] int32: columns [i; j] grouped by i ascending, the
 *        order ddk_complex_create demands; row 1 starts at edge_index_out + cap.  count_out[0] = E.  Status 2: a coordinate that is not finite, found
 *        on the device; E = 0 and nothing is written to edge_index_out.
 *        Limits: 2 <= n <= 65536, 1 <= max_neighbor <= 128, cap >= n * max_neighbor.  Three launches: one workgroup per row (a radix select on the bits
 *        of d2 where more than max_neighbor points lie under the cutoff, however many), a scan of the row counts, the stores.
 *
 *      ddk_radius_graph: torch_cluster.radius_graph(pos, r, max_num_neighbors) for one graph (atom_edge_index, process_mols.py:471).  For every centre i:
 *        the first max_num_neighbors + 1 points j in ascending j with d2 < r^2, self included in that scan; then j == i is dropped.  A centre whose own
 *        index comes after its first max_num_neighbors + 1 in-radius points therefore keeps max_num_neighbors + 1 neighbours (the quirk of LIG_CAP,
 *        csrc/model.h).  edge_index_out [2, cap] int32: columns [neighbour; centre], grouped by centre ascending, neighbours ascending.  count_out[0] = the
 *        E the graph needs.  Status 1: E > cap; nothing past cap columns is written and the columns are not to be read.  Status 2: a coordinate that is
 *        not finite; E = 0, nothing is written.
 *        Limits: 1 <= n <= 65536, 1 <= max_num_neighbors <= 1024, cap >= 1.  Three launches: one wave per centre sweeps j and stops when its quota is
 *        full (brute force, no cell list), a scan of the counts, the same sweep again with the stores.
 *
 *      ddk_ligand_transformation_mask: edge_mask / mask_rotate by the rule of get_transformation_mask, utils/torsion.py:15-45.  bond_index [2, M] int32,
 *        columns 2k and 2k + 1 the two directions (u, v), (v, u) of bond k.  Remove bond k; if the graph falls apart, l is the smaller side, on equal
 *        sizes the side that contains the lowest atom index (networkx's component order under a stable sort).  |l| > 1: the bond is rotatable and the
 *        marked direction is 2k + 1 if u is on l, else 2k: the head rotates, the tail is fixed, which is the orientation ddk_complex_create checks.
 *        edge_mask_out [M] uint8: 1 on the marked columns, every other entry is written 0.  mask_rotate_out [cap_rot, n_lig] uint8: one row per marked
 *        column in ascending column index, 1 on l; rows past R are not touched.  count_out[0] = R.
 *        Status 1: R > cap_rot; edge_mask_out is all 0 (no torsion: the identity fallback), R is reported and mask_rotate_out is not touched.
 *        Status 2: a bond index outside [0, n_lig), a column pair that is not (u, v), (v, u), a bond of an atom with itself or a repeated bond, all found
 *        on the device before an index is used as an address; status 3: the ligand graph is not connected.  With 2 and 3 edge_mask_out is all 0, R = 0
 *        and mask_rotate_out is not touched.  (For a lone counter-ion next to the ligand that is the reference's result too; with a larger second
 *        fragment the reference marks bonds whose row ddk_complex_create refuses, so no table is the honest answer.)
 *        Limits: 1 <= n_lig <= 256, 0 <= M <= 2048 and even, cap_rot >= 1 (bond_index and edge_mask_out may be NULL with M = 0).  One launch of one
 *        workgroup: a thread per bond walks the side of u over the 256-bit adjacency rows. */
int64_t ddk_receptor_knn_graph_workspace(int32_t n, int32_t max_neighbor);
int ddk_receptor_knn_graph(ddk_ctx* ctx, int32_t n, const float* pos, float cutoff, int32_t max_neighbor, int32_t* edge_index_out, int32_t cap,
                           int32_t* count_out /* [2] */, void* workspace, void* stream);
int64_t ddk_radius_graph_workspace(int32_t n, int32_t max_num_neighbors);
int ddk_radius_graph(ddk_ctx* ctx, int32_t n, const float* pos, float r, int32_t max_num_neighbors, int32_t* edge_index_out, int32_t cap,
                     int32_t* count_out /* [2] */, void* workspace, void* stream);
int64_t ddk_ligand_transformation_mask_workspace(int32_t n_lig, int32_t M);
int ddk_ligand_transformation_mask(ddk_ctx* ctx, int32_t n_lig, const int32_t* bond_index, int32_t M, uint8_t* edge_mask_out, uint8_t* mask_rotate_out,
                                   int32_t cap_rot, int32_t* count_out /* [2] */, void* workspace, void* stream);

/* ---- the sampler's random draws, made on the device by a counter-based generator: every number is a pure function of
 *      (seed, complex, sample, step, column), so a pose's draws do not depend on the batch size, on how many ranks share the complex, on the calls made
 *      before, or on any host or torch generator.  (The reference never seeds its RNGs: utils/sampling.py:22-32, 146-164.)  Like the calls above these
 *      take no ddk_complex, allocate nothing and do not synchronise; all data pointers are DEVICE pointers; the work is enqueued on `stream`.
 *
 *      The layout below is an ABI contract: for a given DDK_RNG_LAYOUT the number stream never changes.
 *      Generator: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), csrc/k_philox.h, plain host/device C++.
 *        key = (seed_lo, seed_hi)                        the low and high words of `seed`
 *        counter c0 = stream_lo, c1 = stream_hi          the 64-bit id of the complex, `stream_id` (the Python shim: FNV-1a of its name)
 *                c2 = sample                             the GLOBAL sample index sample0 + b
 *                c3 = purpose << 28 | step << 8 | block  purpose: 4 bits; step < 2^20; block < 256; every block yields 4 words
 *        purpose 0  step noise                 step = the reverse step index      column c uses block c / 4
 *                1  initial torsion uniforms   step = 0                           torsion r uses block r / 4, word r % 4
 *                2  initial rotation           step = 0                           block 0, four normals
 *                3  initial translation        step = 0                           block 0, the first three normals
 *                4  AR pick uniform            step = decoding_idx                block 0, word 0
 *                5  rotation of ar_pos (ar_args.no_randomness, utils/sampling.py:36-46)   step = 0, as purpose 2
 *                6-8  the forward process (ddk_rng_perturbation below): translation, rotation, torsion; step = the draw index
 *                9  conformer matching, the initial population (ddk_conformer_match below)   sample = island * NP + member, step = 0,
 *                                                                                          torsion r uses block r / 4, word r % 4
 *                10 conformer matching, generation g   sample = island * NP + member, step = g; block 0: word 0 -> r1, word 1 -> r2,
 *                                                      word 2 -> the forced crossover index, word 3 OF MEMBER 0 -> the island's mutation factor;
 *                                                      the crossover uniform of component d is word d % 4 of block 1 + d / 4
 *                11 forward time (ddk_rng_forward_times below)   step = the draw index, block 0, word 0: t = the uniform u
 *                12 latent keep (ddk_rng_latent_keep above)      step = the draw index, block 0, word 0: keep iff u >= rate
 *                13 Gumbel noise (DDK_GUMBEL_LAYOUT above)       step = the draw index, block = the latent dimension d: words 0, 1 key the per-node generator
 *                14 AR decoding index (ddk_rng_decoding_index above)   step = the draw index, block 0, word 0: idx = ((word >> 8) * D) >> 24
 *      Words -> draws, in fp32, every operation as written:
 *        uniform      u = (x >> 8) * 2^-24: in [0, 1), exact
 *        torsion      (float)pi * (2u - 1): the inner term is exact, one rounding
 *        normals      a block gives two Box-Muller pairs, from words (0, 1) and (2, 3): u1 = ((x0 >> 8) + 1) * 2^-24 in (0, 1], u2 = (x1 >> 8) * 2^-24,
 *                     r = sqrtf(-2 * logf(u1)), z0 = r * cospif(2 * u2), z1 = r * sinpif(2 * u2), the accurate library functions (no fast-math
 *                     intrinsics).  Column c of a row takes normal c % 4 of block c / 4.  |z| <= sqrt(48 ln 2) = 5.768 by construction; u1 = 1 gives a
 *                     signed zero and never NaN.
 *        rotation     the four normals are the quaternion (x, y, z, w): normalised, then the row-major matrix of scipy's Rotation.from_quat;
 *                     |q|^2 < 2^-60: the identity
 *        translation  tr_sigma * z
 *      The uniforms and torsions are defined bit for bit; a normal is defined up to the last bits of logf / sinpif / cospif of the device library
 *      it was built with (the same library gives the same bits on every call, batch size and rank).
 *
 *      ddk_rng_noise: out [steps, B, n_cols] = what ddk_sample's `noise` argument reads: row (k, b) is step step0 + k of sample sample0 + b; columns at
 *        or past n_active_cols are written 0 (torsion columns a no_torsion run does not use); a step whose three noise_coeff entries are all zero is
 *        written 0 and draws nothing (no_final_step_noise).  noise_coeff: HOST [steps, 3] as ddk_sample takes it, or NULL: every step is active.  One
 *        launch per run of active steps, one memset per run of inactive ones.
 *      ddk_rng_initial: the draws ddk_randomize_position takes: tor_out [B, n_rot] (purpose 1; NULL: not drawn), rot_out [B, 3, 3] (purpose_rot: 2, or 5
 *        for the pose the AR model sees), tr_out [B, 3] = tr_sigma * z (purpose 3; NULL: not drawn).  One launch.
 *      ddk_rng_uniform: out [B], the `uniforms` argument of ddk_ar_decode for latent dimension decoding_idx.  One launch.
 *      Limits: 1 <= B, sample0 >= 0, sample0 + B <= 2^31 - 1, 0 <= step0, 1 <= steps, step0 + steps <= 2^20, 1 <= n_cols <= 1024,
 *      0 <= n_active_cols <= n_cols, 0 <= n_rot <= 1024, 0 <= decoding_idx < 2^20, purpose_rot 2 or 5; anything else, or a NULL output (out, rot_out),
 *      is DDK_ERR_INVALID with a ddk_last_error text, and nothing is enqueued. */
#define DDK_RNG_LAYOUT 1
int ddk_rng_noise(ddk_ctx* ctx, uint64_t seed, uint64_t stream_id, int32_t sample0, int32_t B, int32_t step0, int32_t steps, int32_t n_cols,
                  int32_t n_active_cols, const float* noise_coeff /* HOST [steps, 3] or NULL */, float* out /* [steps, B, n_cols] */, void* stream);
int ddk_rng_initial(ddk_ctx* ctx, uint64_t seed, uint64_t stream_id, int32_t sample0, int32_t B, int32_t n_rot, float tr_sigma,
                    int32_t purpose_rot /* 2 or 5 */, float* tor_out /* [B, n_rot] or NULL */, float* rot_out /* [B, 3, 3] */,
                    float* tr_out /* [B, 3] or NULL */, void* stream);
int ddk_rng_uniform(ddk_ctx* ctx, uint64_t seed, uint64_t stream_id, int32_t sample0, int32_t B, int32_t decoding_idx, float* out /* [B] */,
                    void* stream);

/* ---- the forward half of the diffusion and the score-matching loss: what the reference's validation pass (test_epoch, utils/training.py) is made of.
 *      NoiseTransform.apply_noise (datasets_utils/pdbbind.py:40-57) noises the true pose and records the three score targets; loss_function
 *      (utils/training.py:14-61) sets the model's three scores against them.  Like the ddk_rng_* calls these take no ddk_complex, allocate nothing, do not
 *      synchronise and enqueue on `stream`; all data pointers are DEVICE pointers unless marked HOST; a broken limit is DDK_ERR_INVALID with a
 *      ddk_last_error text and nothing is enqueued.  No float atomics: the results are bit-identical run to run.
 *
 *      ddk_so3_rows: rows of the IGSO(3) tables of utils/so3.py, computed in fp64 instead of read from a cache (MIN_EPS 0.01, MAX_EPS 2, N_EPS 1000,
 *        X_N 2000, L = 2000 terms).  Row i of the call has eps = 10 ** linspace(log10 0.01, log10 2, 1000)[eps_idx[i]] (the grid is computed in fp64 on the
 *        host) on the angles omega_j = pi (j + 1) / 2000.  cdf_out [n_rows, 2000] = _cdf_vals (the cumulative sum of _density(_expansion, marginal) times
 *        pi / 2000, so3.py:21-30, 56-58), score_out [n_rows, 2000] = _score_norms (_score, so3.py:35-43, 59), exp_score_norm_out [n_rows] =
 *        _exp_score_norms (so3.py:61).  Every (row, omega) element is accumulated by one thread with l ascending and every term as the reference writes
 *        it, the order that reproduces the reference's tables bit for bit on the host; the device differs from them by the last bits of its sin, cos and
 *        exp.  score_out is written as the reference computes it, inf and NaN included: where the density vanishes (pdf below about 1e-9 of the row's
 *        maximum) the series cancels and both tables are numerical noise, which no reachable draw reads.  exp_score_norm_out sums score^2 pdf over the
 *        entries whose score is FINITE and whose expansion stands above the rounding noise of its own sum, |f| > 2^-40 sum_l |term_l|, only; sum(pdf)
 *        runs over all entries.  (score^2 pdf = dSigma^2 (1 - cos omega) / (pi f) is unbounded as a cancelled f comes close to 0: without the second
 *        condition one entry in a few hundred thousand outweighs 1e-10 of its row, as rows 44 and 55 of the reference's own table show.  The entries
 *        left out carry less than 1e-10 of the sum; the result is within 1e-9 of the reference's on every row.)
 *        Limits: 1 <= n_rows <= 4096, every eps_idx in [0, 1000), duplicates allowed, at least one output not NULL.  One launch per 256 rows, one
 *        workgroup per row.
 *
 *      ddk_torus_score: torus.score(x, sigma) (utils/torus.py:43-52) per element without the 5001 x 5001 table: in fp64, x wrapped to [-pi, pi), |x|
 *        quantised to the grid 10 ** linspace(-5, 0, 5001) * pi as there (natural log, clip to [0, 5000], round half to even), grad / p of torus.py:11-22
 *        with N = 100 evaluated at that grid point and sigma = 10 ** linspace(log10 3e-3, log10 2, 5001)[sigma_idx] * pi, times -sign(x), rounded once to
 *        fp32.  x == 0 gives 0; where p underflows to 0 the result is NaN, as in the reference's table (x index 5000 at sigma index 0); an x that is not
 *        finite gives NaN.  sigma_idx is a HOST quantity (torus.py:49-51 in fp64 on the host's sigma), so a rounding tie cannot differ between host and
 *        device.  Limits: n >= 0, 0 <= sigma_idx <= 5000.  One launch.
 *
 *      ddk_rng_perturbation: one noising of the global samples sample0 .. sample0 + B - 1 at one noise level: the three updates ddk_se3_update takes and
 *        their score targets, from the generator above (DDK_RNG_LAYOUT 1) with three more purposes; `draw` sits in the step field, so a sample can be
 *        noised independently up to 2^20 times:
 *          purpose 6  forward translation   step = draw   block 0, the first three normals z: tr_update = tr_sigma * z
 *                  7  forward rotation      step = draw   block 0, normals 0..2 = the axis a; block 1, word 0 = the uniform u
 *                  8  forward torsion       step = draw   torsion r uses normal r % 4 of block r / 4: tor_update = tor_sigma * z
 *        tr_score = -tr_update / tr_sigma^2 (fp32).  rot_update = a / |a| * omega in fp64, rounded once to fp32, with omega = np.interp(u, so3_cdf_row,
 *        omegas) (so3.sample, so3.py:69-80), clamped at both ends like NumPy's, the bracket found by bisection for the first cdf[j] >= u; |a|^2 < 2^-60:
 *        rot_update = rot_score = 0.  rot_score = np.interp(omega, omegas, so3_score_row) * rot_update / omega (so3.score_vec, so3.py:83-88) in fp64,
 *        rounded once.  tor_score = ddk_torus_score's arithmetic on tor_update at torus_sigma_idx.  so3_cdf_row / so3_score_row [2000]: one row of
 *        ddk_so3_rows, for so3_eps_index(rot_sigma).  None of the purposes 0-5 is touched: every existing draw keeps its bits.
 *        out: caller-owned arrays; the updates may not be NULL (tor_update may with n_rot = 0), a score member may be (not computed; so3_score_row may
 *        then be NULL too).  Limits: those of ddk_rng_initial (1 <= B, sample0 >= 0, sample0 + B <= 2^31 - 1, 0 <= n_rot <= 1024), 0 <= draw < 2^20,
 *        tr_sigma, tor_sigma > 0, 0 <= torus_sigma_idx <= 5000.  One launch.
 *
 *      ddk_score_matching_loss: out [B, 6] = {tr_loss, rot_loss, tor_loss, tr_base_loss, rot_base_loss, tor_base_loss} per sample, the terms of
 *        loss_function(..., apply_mean=False): tr = mean_3((pred - score)^2 sigma^2), rot = mean_3(((pred - score) / so3_score_norm)^2),
 *        tor = sum_r((pred - score)^2 / torus_score_norm2) / (n_rot + 1e-4); the base terms are the same expressions with pred = 0.  tor arrays [B, n_rot];
 *        n_rot = 0 or tor_pred = NULL gives 0 for the two torsion terms.  One wave per sample, fp64 inside, a fixed reduction order, each term rounded
 *        once to fp32.  Limits: 1 <= B, 0 <= n_rot <= 1024, the three scalars > 0.  One launch. */
int ddk_so3_rows(ddk_ctx* ctx, int32_t n_rows, const int32_t* eps_idx /* HOST [n_rows], each in [0, 1000) */,
                 double* cdf_out /* DEVICE [n_rows, 2000] or NULL */, double* score_out /* DEVICE [n_rows, 2000] or NULL */,
                 double* exp_score_norm_out /* DEVICE [n_rows] or NULL */, void* stream);
int ddk_torus_score(ddk_ctx* ctx, int64_t n, const float* x /* DEVICE [n] */, int32_t sigma_idx /* in [0, 5000] */, float* score_out /* DEVICE [n] */,
                    void* stream);
typedef struct ddk_perturbation {           /* caller-owned DEVICE arrays; updates may not be NULL, a score member may be */
  float *tr_update, *rot_update, *tor_update;   /* [B,3] [B,3] [B,n_rot]  what ddk_se3_update takes */
  float *tr_score, *rot_score, *tor_score;      /* [B,3] [B,3] [B,n_rot]  data.tr_score / rot_score / tor_score */
} ddk_perturbation;
int ddk_rng_perturbation(ddk_ctx* ctx, uint64_t seed, uint64_t stream_id, int32_t sample0, int32_t B, int32_t draw, int32_t n_rot, float tr_sigma,
                         float tor_sigma, int32_t torus_sigma_idx, const double* so3_cdf_row, const double* so3_score_row /* DEVICE [2000] each */,
                         const ddk_perturbation* out, void* stream);
int ddk_score_matching_loss(ddk_ctx* ctx, int32_t B, int32_t n_rot, const float* tr_pred, const float* rot_pred, const float* tor_pred,
                            const float* tr_score, const float* rot_score, const float* tor_score, float tr_sigma, float so3_score_norm,
                            float torus_score_norm2, float* out /* [B, 6] */, void* stream);

/* ---- the same three steps for a RAGGED batch: G graphs that are different complexes, each at its own diffusion time, which is what the reference's
 *      training loader delivers (NoiseTransform per complex, then collation; train_epoch, utils/training.py:96-135).  Like the calls above these take no
 *      ddk_complex, allocate nothing, do not synchronise and enqueue on `stream`; a broken limit or a NULL required argument is DDK_ERR_INVALID with a
 *      ddk_last_error text that names it, and nothing is enqueued.  The per-graph tables ([G] or [G + 1]) are DEVICE arrays the host side of the call never
 *      reads; the caller (the Python shim checks them on the host before the one copy that uploads them) is responsible for them, and every entry is
 *      checked on the device before it becomes an address or a table index.  No float atomics; a graph's results do not depend on the other graphs of the
 *      batch, on its place in it or on G.
 *      Ragged torsion arrays are flat [T] with the prefix tor_ptr [G + 1] of the rotor counts R_g (tor_ptr[0] = 0, tor_ptr[G] = T, R_g = 0 allowed).
 *
 *      ddk_rng_perturbation_batch: one noising (draw index `draw`) of G graphs: graph g is the global sample sample[g] of stream stream_id[g] under `seed`
 *        at the noise level tr_sigma[g], tor_sigma[g], torus_sigma_idx[g] and row so3_row[g] of the caller's so3_cdf_rows / so3_score_rows [n_rows, 2000]
 *        (rows of ddk_so3_rows in any order).  DDK_RNG_LAYOUT 1, purposes 6-8 exactly as for ddk_rng_perturbation.  out: tr_update, rot_update, tr_score,
 *        rot_score [G, 3]; tor_update, tor_score [T]; the score members (and tor_update with T = 0) may be NULL.  The values of graph g are bit for bit
 *        those of ddk_rng_perturbation(seed, stream_id[g], sample0 = sample[g], B = 1, draw, n_rot = R_g, ...) with g's scalars and rows.  The sigma of a
 *        torus index is read from a 5001-entry table the FIRST batch call on a device computes on the host and uploads (40 kB, a blocking copy, once per
 *        process and device), so that it is the host's number as in the single call.  A graph with a broken entry (tor_ptr not a range of [0, T], R_g >
 *        1024, an index outside its table, a sample < 0, a sigma that is not positive and finite) gets NaN in its tr_update / rot_update rows and nothing
 *        else.  Limits: 1 <= G <= 65536, 0 <= T <= 1024 G, 0 <= draw < 2^20, 1 <= n_rows <= 4096.  One launch, one workgroup per graph.
 *
 *      ddk_rng_forward_times: the diffusion time of each of n complexes for one noising, t_out[i] = the uniform of purpose 11 for (seed, stream_id[i],
 *        sample, draw): in [0, 1), i.e. NoiseTransform's Beta(alpha, beta) draw for the reference's default alpha = beta = 1.  A HOST function (stream_id and
 *        t_out are HOST arrays, no kernel, also on a host-only context): the noise levels of a batch are host scalars (the table indices are computed
 *        from them), the generator is plain integer code and the word -> uniform conversion is exact, so the device has nothing to add.
 *
 *      ddk_modify_conformer_batch: modify_conformer (utils/diffusion_utils.py) per graph: the rigid move by (tr_update[g], rot_update[g]) about the
 *        graph's centroid, the torsion rotations in bond order on the already-updated coordinates, the Kabsch re-alignment of the flexed conformer onto
 *        the rigid one.  pos / pos_out [N, 3] with the atoms of graph g at node_ptr[g] .. node_ptr[g + 1]; rot_bonds [T, 2] graph-local (u, v) and
 *        mask_rotate, the graphs' [R_g, n_g] byte blocks back to back with graph g's at mask_ptr[g] (mask_bytes in all), as ddk_conformer_rmsd takes them.
 *        tor_update = NULL: rigid moves only (the rotor tables may then be NULL).  One workgroup per graph with the arithmetic of ddk_se3_update: centred
 *        coordinates, fp64 centroid sums, Horn's closed form; pos_out of graph g is bit for bit ddk_se3_update's with B = 1 on a ddk_complex of that ligand
 *        and the same updates; a graph with R_g = 0 gets the rigid move.  status_out [G]: 0 done; 2 a bond index outside [0, n_g) or u == v; 3 a
 *        coordinate that is not finite; 4 a node_ptr / tor_ptr / mask_ptr entry that is no range of its array, n_g outside [1, 256], R_g outside [0, 1024]
 *        or a mask block that is not R_g * n_g bytes: all found before an index is used as an address; with 2, 3 or 4 the graph's rows of pos_out are
 *        not written.  Limits: 1 <= G <= 65536, G <= N <= 256 G, 0 <= T <= 1024 G, mask_bytes >= 0.  One launch.
 *
 *      ddk_score_matching_loss_batch: out [G, 6], row g = ddk_score_matching_loss(B = 1, n_rot = R_g, ...) bit for bit with the graph's own tr_sigma[g],
 *        so3_score_norm[g], torus_score_norm2[g] (one torus norm per graph: every torsion edge of a graph carries the graph's tor_sigma).  tor_pred = NULL
 *        or R_g = 0: the graph's torsion terms are 0.  A graph with a tor_ptr pair that is no range of [0, T], R_g > 1024 or a scalar that is not positive
 *        gets a row of NaN.  One launch, one wave per graph.
 *      ddk_score_matching_loss_batch_backward: from grad [G, 3], the gradient of the three loss columns, the gradients of the predictions, each written
 *        only where its destination is not NULL: grad_tr_pred [G, 3] = 2 (pred - score) tr_sigma^2 / 3 * grad[g][0], grad_rot_pred [G, 3] = 2 (pred -
 *        score) / so3_score_norm^2 / 3 * grad[g][1], grad_tor_pred [T] = 2 (pred - score) / torus_score_norm2 / (R_g + 1e-4) * grad[g][2]; element-wise,
 *        fp64 inside, one rounding.  One launch (none if nothing is asked for).
 *      Limits of both: 1 <= G <= 65536, 0 <= T <= 1024 G. */
int ddk_rng_perturbation_batch(ddk_ctx* ctx, uint64_t seed, int32_t G, const uint64_t* stream_id /* DEVICE [G] */, const int32_t* sample /* DEVICE [G] */,
                               const int32_t* tor_ptr /* DEVICE [G + 1] */, int32_t T, int32_t draw, const float* tr_sigma, const float* tor_sigma,
                               const int32_t* torus_sigma_idx, const int32_t* so3_row /* DEVICE [G] each */, int32_t n_rows,
                               const double* so3_cdf_rows, const double* so3_score_rows /* DEVICE [n_rows, 2000] each */, const ddk_perturbation* out,
                               void* stream);
int ddk_rng_forward_times(ddk_ctx* ctx, uint64_t seed, int32_t n, const uint64_t* stream_id /* HOST [n] */, int32_t sample, int32_t draw,
                          float* t_out /* HOST [n] */);
int ddk_modify_conformer_batch(ddk_ctx* ctx, int32_t G, int32_t N, const float* pos /* [N, 3] */, const int32_t* node_ptr /* [G + 1] */, int32_t T,
                               const int32_t* rot_bonds /* [T, 2] */, const uint8_t* mask_rotate /* [mask_bytes] */, const int32_t* mask_ptr /* [G + 1] */,
                               int32_t mask_bytes, const int32_t* tor_ptr /* [G + 1] */, const float* tr_update, const float* rot_update /* [G, 3] */,
                               const float* tor_update /* [T] or NULL */, float* pos_out /* [N, 3] */, int32_t* status_out /* [G] */, void* stream);
/* ddk_randomize_position_batch: randomize_position(..., unbatched=True) (utils/sampling.py:12-34) for G DIFFERENT ligands in one collated table, the start
 *   poses of an AR training batch.  pos / pos_out, node_ptr, rot_bonds, mask_rotate, mask_ptr, mask_bytes, tor_ptr and T as ddk_modify_conformer_batch takes
 *   them; stream_id [G] (uint64) and sample [G] (int32): graph g is the global sample sample[g] of stream stream_id[g] under `seed`.  The workgroup of graph g
 *   makes the draws of ddk_rng_initial itself (DDK_RNG_LAYOUT 1, purposes 1, 2 and 3: R_g torsion angles, the rotation, tr_sigma_max * z) and applies
 *   ddk_randomize_position's arithmetic: the torsion rotations in bond order (axis pos_u - pos_v, pivot pos_v, a zero angle skipped), then
 *   (pos - centroid) R^T + tr.  pos_out of graph g is BIT FOR BIT what ddk_rng_initial(seed, stream_id[g], sample0 = sample[g], B = 1, n_rot = R_g,
 *   tr_sigma_max) followed by ddk_randomize_position gives that ligand alone, whatever else is in the batch and wherever the graph stands in it.
 *   tor_ptr = NULL: no torsions are drawn (no_torsion; the rotor tables may then be NULL).  status_out [G] and the rule that a graph with a status other
 *   than 0 is not written are ddk_modify_conformer_batch's; a sample < 0 is status 4.  Limits: those of ddk_modify_conformer_batch; tr_sigma_max finite and
 *   >= 0.  One launch, one workgroup per graph, no draw array in memory. */
int ddk_randomize_position_batch(ddk_ctx* ctx, uint64_t seed, int32_t G, int32_t N, const float* pos /* [N, 3] */, const int32_t* node_ptr /* [G + 1] */,
                                 int32_t T, const int32_t* rot_bonds /* [T, 2] */, const uint8_t* mask_rotate /* [mask_bytes] */,
                                 const int32_t* mask_ptr /* [G + 1] */, int32_t mask_bytes, const int32_t* tor_ptr /* [G + 1] or NULL */,
                                 const uint64_t* stream_id /* DEVICE [G] */, const int32_t* sample /* DEVICE [G] */, float tr_sigma_max,
                                 float* pos_out /* [N, 3] */, int32_t* status_out /* [G] */, void* stream);
int ddk_score_matching_loss_batch(ddk_ctx* ctx, int32_t G, const int32_t* tor_ptr /* [G + 1] */, int32_t T, const float* tr_pred, const float* rot_pred,
                                  const float* tor_pred, const float* tr_score, const float* rot_score, const float* tor_score,
                                  const float* tr_sigma, const float* so3_score_norm, const float* torus_score_norm2 /* DEVICE [G] each */,
                                  float* out /* [G, 6] */, void* stream);
int ddk_score_matching_loss_batch_backward(ddk_ctx* ctx, int32_t G, const int32_t* tor_ptr, int32_t T, const float* grad /* [G, 3] */, const float* tr_pred,
                                           const float* rot_pred, const float* tor_pred, const float* tr_score, const float* rot_score,
                                           const float* tor_score, const float* tr_sigma, const float* so3_score_norm, const float* torus_score_norm2,
                                           float* grad_tr_pred /* [G, 3] or NULL */, float* grad_rot_pred /* [G, 3] or NULL */,
                                           float* grad_tor_pred /* [T] or NULL */, void* stream);

/* ---- conformer matching: fit the torsion angles of a generated conformer so that, after the optimal rigid fit, it lies as close as possible to the true
 *      pose (datasets_utils/conformer_matching.py, called from get_lig_graph_with_matching, datasets_utils/process_mols.py:280-311; the reference trains and
 *      validates on matched conformers and reports rmsd_matching per dataset).  Like ddk_ligand_automorphisms these calls take no ddk_complex, allocate
 *      nothing and do not synchronise; all data pointers are DEVICE pointers; the work is enqueued on `stream`; a status other than 0 is a result (the call
 *      returns DDK_OK); a broken limit or a NULL required argument is DDK_ERR_INVALID with a ddk_last_error text and nothing is enqueued.  No float atomics:
 *      the results are bit-identical run to run and a pure function of (ligand, target, options).
 *
 *      The objective (ddk_conformer_rmsd evaluates it alone, rmsd_out[m] for the M vectors torsions [M, n_rot]): modify_conformer_torsion_angles
 *        (utils/torsion.py:48-68) followed by the RMSD after the optimal proper rotation and translation.  For rotor k in order, on the already-updated
 *        coordinates, the atoms with mask_rotate[k] rotate about pos[v] by the angle theta_k around (pos[u] - pos[v]) / |pos[u] - pos[v]|; a rotor with
 *        theta_k == 0 is skipped.  rot_bonds [n_rot, 2] = the (u, v) of the rotatable bonds, bond_index[:, edge_mask].T, and mask_rotate [n_rot, n_lig] its
 *        rows, as ddk_ligand_transformation_mask produces them.  The torsions are RELATIVE increments applied to pos0, where the reference sets absolute
 *        dihedral angles through RDKit: both reach the same set of shapes, so the minimum is the same, the minimiser differs by the conformer's own angles.
 *        atom_mask [n_lig] uint8 (NULL = all atoms): the atoms that enter the fit and the RMSD (the reference matches after RemoveHs); masked-out atoms
 *        are moved like the others and written to pos_out.  The rotor chain runs in fp32 on centred coordinates, the centroids, the covariance and the
 *        squared norms are fp64 sums, and msd = (sum |a|^2 + sum |b|^2 - 2 lambda_max) / m with lambda_max the top eigenvalue of Horn's 4 x 4 matrix.
 *      Status (status_out[0] / count_out[1]): 0 done; 2 a bond index outside [0, n_lig), u == v, mask_rotate[k][u] != 0 or mask_rotate[k][v] == 0 (the two
 *        asserts of the reference), or fewer than 3 kept atoms; 3 a coordinate of pos0 or target that is not finite.  All found on the device before an
 *        index is used as an address.  With 2 or 3 nothing but status_out / count_out is written (count_out = {0, status}).
 *
 *      ddk_conformer_match: the reference's differential_evolution(f, [(-pi, pi)] * n_rot, maxiter, popsize, mutation=(0.5, 1), recombination=0.8)
 *        (conformer_matching.py:39-41: strategy best1bin, tol 0.01, a polish at the end), with three deliberate differences:
 *          updating   generation-synchronous: every trial of generation g is built from the population of generation g - 1 (scipy's own
 *                     updating='deferred'; the reference runs 'immediate')
 *          bounds     a trial component outside the bounds is wrapped into [-pi, pi): the objective is 2 pi-periodic (scipy redraws the component)
 *          population independent uniform torsions (purpose 9 above), not a Latin hypercube, and member 0 of island 0 is theta = 0: selection is elitist,
 *                     so rmsd_out[1] <= rmsd_out[0] always
 *        n_islands independent populations of NP = max(5, popsize * n_rot) members each (no migration; island j draws the same numbers whatever
 *        n_islands is, so the search's result BEFORE THE POLISH is never worse with more islands; the polish then starts from a possibly different vector, so
 *        after it that holds only as a rule); the result is the best member over the islands, ties to the lowest island, then member.
 *        Generation g = 1 .. maxiter of an island, from the population and costs of generation g - 1:
 *          stop       mean and standard deviation (population form, / NP) of the NP costs in fp64; std <= tol * |mean| stops the island: this and every later
 *                     generation leave it unchanged (tested before generation 1 too).  count_out[0] = the largest number of generations an island ran.
 *          best       the member of the lowest cost, ties to the lowest index
 *          F          0.5f + 0.5f * u, u the uniform of word 3 of block 0 of the island's member 0: one factor per (island, generation)
 *          member i   r1 = ((x0 >> 8) * (NP - 1)) >> 24, plus 1 if >= i; r2 = ((x1 >> 8) * (NP - 2)) >> 24, plus 1 if >= min(i, r1), then plus 1 if
 *                     >= max(i, r1): r1 != r2, both != i, integer arithmetic only; forced = ((x2 >> 8) * n_rot) >> 24
 *          trial      component d = wrap(fmaf(F, pop[r1][d] - pop[r2][d], pop[best][d])) if d == forced or its uniform < 0.8f, else pop[i][d];
 *                     wrap(t) = t - 2 pi floor((t + pi) / (2 pi)) in fp32, folded once more if the rounding left it outside [-pi, pi)
 *          selection  the trial replaces member i if its cost <= the member's (a NaN cost never does)
 *        Polish (instead of scipy's L-BFGS-B): a compass search from the best vector, h = 0.5: evaluate the 2 n_rot candidates theta +- h e_d (wrapped),
 *        take the best one (ties to the lowest d, + before -) if it is strictly better, otherwise halve h; stop at h < 1e-4 or after polish_iters
 *        iterations.  No random numbers.
 *        Outputs: torsions_out [n_rot] the best vector; pos_out [n_lig, 3] the matched conformer in the target's frame (the AlignMolConformers step of
 *        process_mols.py:305-307: the pose the reference stores as the ligand's pos); rmsd_out [2] = {the rigid fit with all torsions 0, the matched
 *        RMSD = rmsd_matching}; count_out [2] = {generations run, status}.  n_rot = 0 is valid: no generation, pos_out = the rigid fit, both RMSDs
 *        equal (the reference's `if rotable_bonds:`).
 *        opt: a HOST struct.  workspace: ddk_conformer_match_workspace(...) bytes of device memory, 16-byte aligned, contents irrelevant before and after
 *        (a host function, no context; -1 if a limit is broken).  Launches: one validation, maxiter + 1 generations over a fixed grid of one wave per
 *        member (the boundary between two launches is the only ordering between workgroups: no grid barrier, no persistent kernel), one workgroup that
 *        picks the best member, polish_iters launches of one wave per neighbour (those left after the polish has ended return at once), one workgroup
 *        for the final fit.
 *      Limits: 3 <= n_lig <= 256, 0 <= n_rot <= 128, 1 <= popsize <= 64, 0 <= maxiter <= 1000, 0 <= polish_iters <= 1024, 1 <= n_islands <= 16,
 *      tol >= 0, 1 <= M <= 65536, NP <= 8192. */
typedef struct ddk_match_options {
  int32_t popsize, maxiter;
  float tol;
  int32_t polish_iters, n_islands;
  uint64_t seed, stream_id;
} ddk_match_options;
int64_t ddk_conformer_match_workspace(int32_t n_lig, int32_t n_rot, int32_t popsize, int32_t n_islands);
int ddk_conformer_rmsd(ddk_ctx* ctx, int32_t n_lig, const float* pos0, const float* target, const uint8_t* atom_mask,
                       const int32_t* rot_bonds /* [n_rot, 2] (u, v) */, const uint8_t* mask_rotate /* [n_rot, n_lig] */, int32_t n_rot,
                       int32_t M, const float* torsions /* [M, n_rot] */, float* rmsd_out /* [M] */, int32_t* status_out /* [1] */, void* stream);
int ddk_conformer_match(ddk_ctx* ctx, int32_t n_lig, const float* pos0, const float* target, const uint8_t* atom_mask,
                        const int32_t* rot_bonds, const uint8_t* mask_rotate, int32_t n_rot, const ddk_match_options* opt /* HOST */,
                        float* torsions_out /* [n_rot] */, float* pos_out /* [n_lig, 3] */, float* rmsd_out /* [2] */, int32_t* count_out /* [2] */,
                        void* workspace, void* stream);

/* ---- a1-a2: the reverse-diffusion loop of sampling()  utils/sampling.py:105-198 for one batch:
 *      per step  perturb = score_coeff*score + noise_coeff*z  (coefficients are the host scalars of
 *      sampling.py:137-192, including the low-temperature variant), then ddk_se3_update.
 *      t [steps,3]; score_coeff / noise_coeff [steps,3] HOST arrays (tr,rot,tor);
 *      noise: DEVICE array [steps, B, 6 + n_rot] of N(0,1) draws (tr xyz, rot xyz, tor...), or NULL = zeros.
 *      pos [B,n_lig,3] is updated in place.  No host synchronisation inside. */
int ddk_sample(ddk_ctx* ctx, ddk_complex* cx, int32_t B, int32_t steps, const float* t, const float* score_coeff,
               const float* noise_coeff, const float* noise, float* pos, void* stream);

/* ---- ddk_sample that also RECORDS the trajectory on the device: what utils/sampling.py:224-228 hands to the visualisation_list
 *      per batch (evaluate.py --save_visualisation, evaluate.py:236-247, 344-392) and, per step, the quantities of
 *      utils/sampling.py:113-135 (scores, after the classifier-free guidance combination on guided steps) and :137-198 (the
 *      tr / rot / tor perturbations passed to modify_conformer_batch).  The record is written by the launches ddk_sample makes
 *      anyway: no launch and no copy is added per step (one device-to-device copy of the start poses before the loop), and there
 *      is still no host synchronisation inside.  Same arguments, arithmetic and refusals as ddk_sample (steps < 1, B above the
 *      complex's max_batch, a confidence_mode context); the poses come out bit-identical with and without a record.
 *      rec: caller-owned DEVICE arrays, any member may be NULL (= not recorded); rec == NULL or all members NULL is ddk_sample:
 *        pos         [steps + 1, B, n_lig, 3]  row k = the poses BEFORE step k, row steps = the final poses (= pos on return)
 *        scores      [steps, B, 6 + n_rot]     tr xyz, rot xyz, tor... exactly as step k's update consumed them
 *        perturb     [steps, B, 6 + n_rot]     score_coeff * score + noise_coeff * z of step k
 *        edge_counts [steps, 4] int32          batch totals E_ll, E_lr, E_rr, E_rl of the graph step k's forward ran on
 *                                              (ddk_last_graph_stats out[0..3], without its synchronisation)
 *      The column layout 6 + n_rot is the noise argument's; the torsion columns are zero on a no_torsion context.  The arrays
 *      must not overlap pos or each other and are complete once the stream has passed the call. */
typedef struct ddk_trajectory {
  float* pos;
  float* scores;
  float* perturb;
  int32_t* edge_counts;
} ddk_trajectory;
int ddk_sample_trajectory(ddk_ctx* ctx, ddk_complex* cx, int32_t B, int32_t steps, const float* t, const float* score_coeff,
                          const float* noise_coeff, const float* noise, float* pos, const ddk_trajectory* rec, void* stream);

/* ---- graph construction alone (score_model.py:310-344 build_lig_conv_graph, :346-373 build_rec_conv_graph, :375-408
 *      build_cross_conv_graph, merged as in :218-225): for B poses of the complex at diffusion time t_tr, the ONE edge list the
 *      conv layers consume, in the reference's group order [lig-lig | lig->rec | rec-rec | rec->lig(flipped)], every group sorted
 *      by edge_src.  Row convention of tensor_layers.py:147-159: edge_src = node that RECEIVES the message (scatter index),
 *      edge_dst = node whose features enter the tensor product; node numbering [ligand atoms of all samples | residues of all
 *      samples].  lig-lig = covalent bonds + radius_graph(lig_max_radius, max_num_neighbors = 32: up to 33 kept per atom, see csrc/model.h LIG_CAP); cross cutoff = 3 sigma_tr(t_tr) + 20
 *      (dynamic_max_cross) or cross_max_distance.  edge_src_out / edge_dst_out: device [cap] int32; group_offsets_out: device [5]
 *      int32 (offsets of the four groups, [4] = E).  DDK_ERR_INVALID when cap is below the complex' worst case
 *      (ddk_last_graph_stats out[7]); no host synchronisation inside. */
int ddk_build_graph(ddk_ctx* ctx, ddk_complex* cx, int32_t B, const float* lig_pos, float t_tr, int32_t* edge_src_out,
                    int32_t* edge_dst_out, int64_t cap, int32_t* group_offsets_out, void* stream);

/* ---- introspection for tests / benches ------------------------------------------------------ */
/* Copies the last forward's edge counts into out[12] (HOST, synchronises the stream): [0..3] = E_ll, E_lr, E_rr, E_rl of the reference
 * graph, [4] = edges of the shared receptor-receptor copy (layer-0 de-duplication), [5] = E, [6] = capacity overflow flag,
 * [7] = edge capacity, [8..10] = receptor-receptor edges inside the heads' backward receptive field one / two / three layers below
 * the last conv layer (= E_rr when the pruning is off), [11] != 0: the graph's count and fill kernels disagreed about a sample's edge count in some
 * forward since the complex was created (an internal consistency guard: the edge list of that forward is not to be trusted). */
int ddk_last_graph_stats(ddk_ctx* ctx, ddk_complex* cx, int64_t* out, void* stream);
/* Node features after the conv stack of the last forward: lig [B*n_lig, 84], rec [B*n_rec, 84] (device ptrs, may be NULL).
 * rec_out != NULL requires ddk_set_keep_receptor_features(on) before that forward (DDK_ERR_STATE otherwise). */
int ddk_last_node_features(ddk_ctx* ctx, ddk_complex* cx, int32_t B, float* lig_out, float* rec_out, void* stream);

/* ---- measurement: HIP-event timing of every fused TP-conv launch on the stream it is launched on (bench.py's
 *      roofline leg).  ddk_profile_read synchronises, then fills per conv layer l (n >= 5 * num_conv_layers doubles, HOST):
 *      out[5l] = total kernel ms, out[5l+1] = launches, out[5l+2] = edges the launches evaluated, out[5l+3] = edges they would
 *      have evaluated without the receptive-field pruning (layer-0 de-duplication and the last layer's ligand-only evaluation
 *      still applied: the round-1 accounting), out[5l+4] = edges the reference evaluates in that layer (all of E every layer). */
int ddk_profile_enable(ddk_ctx* ctx, int32_t on);
int ddk_profile_read(ddk_ctx* ctx, double* out, int32_t n);
/*      The same records per FORWARD, in launch order (a sampling loop of K steps = K consecutive forwards): out[4f] = conv kernel ms
 *      of forward f (its conv launches together), out[4f+1] = edges they evaluated, out[4f+2] = edges without the receptive-field
 *      pruning, out[4f+3] = cross edges lig->rec of the forward's graph.  Returns the number of forwards recorded since
 *      ddk_profile_enable(on) (at most max_forwards are written), or a negative error code. */
int ddk_profile_read_forwards(ddk_ctx* ctx, double* out, int32_t max_forwards);

#ifdef __cplusplus
}
#endif
#endif /* DDK_H */
