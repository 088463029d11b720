// C-ABI entry points (include/ddk.h).  This file keeps the context (fail, hip_fail, ctx_malloc ... ensure, find_w), ddk_create, ddk_destroy,
// ddk_load_weights, ddk_finalize_weights, the operator entry points (ddk_tp_forward, ddk_conv_forward, ...) and the export / debug hooks.
// What turns a state dict into a ConvLayerDev (tile tables, MFMA fragments, f16-limb records) is conv_pack.hip.
#include <string.h>

#include "model.h"
#include "k_philox.h"
#include "k_tp_shape.h"

using namespace ddk;

namespace ddk {

int fail(ddk_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

int hip_fail(ddk_ctx* ctx, hipError_t e, const char* what) {
  return fail(ctx, DDK_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

hipError_t ctx_malloc(ddk_ctx* ctx, void** p, size_t bytes) {
  *p = nullptr;
  if (ctx->alloc_limit > 0 && ctx->dev_bytes + (int64_t)bytes > ctx->alloc_limit) { ctx->alloc_refusals++; return hipErrorOutOfMemory; }
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return e; }      // (the sticky error is consumed: the context stays usable)
  ctx->dev_bytes += (int64_t)bytes;
  ctx->dev_sizes[*p] = bytes;
  return hipSuccess;
}

void ctx_free(ddk_ctx* ctx, void* p) {
  if (!p) return;
  auto it = ctx->dev_sizes.find(p);
  if (it != ctx->dev_sizes.end()) { ctx->dev_bytes -= (int64_t)it->second; ctx->dev_sizes.erase(it); }
  hipFree(p);
}

void* dev_alloc(ddk_ctx* ctx, size_t bytes) {
  void* p = nullptr;
  if (bytes == 0) bytes = 16;
  if (ctx_malloc(ctx, &p, bytes) != hipSuccess) {
    // memory pressure: the chunks parked in the pool are the context's own slack - hand them back and try once more
    if (pool_evict_idle(ctx, true) == 0 || ctx_malloc(ctx, &p, bytes) != hipSuccess) return nullptr;
  }
  ctx->dev_allocs.push_back(p);
  return p;
}

float* dev_upload(ddk_ctx* ctx, const std::vector<float>& v) {
  float* p = (float*)dev_alloc(ctx, v.size() * sizeof(float));
  if (p && !v.empty()) {
    if (hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  }
  return p;
}

int ensure(ddk_ctx* ctx, void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes && *p) return DDK_OK;
  if (*p) {
    ctx_free(ctx, *p);
    *p = nullptr;
    *cap = 0;
  }
  size_t want = bytes + bytes / 4 + 256;
  if (ctx_malloc(ctx, p, want) != hipSuccess) {
    if (pool_evict_idle(ctx, true) == 0 || ctx_malloc(ctx, p, want) != hipSuccess)
      return fail(ctx, DDK_ERR_NOMEM, "out of device memory: workspace of " + std::to_string(want) + " B (context holds " + std::to_string(ctx->dev_bytes) + " B" +
                  (ctx->alloc_limit > 0 ? ", debug limit " + std::to_string(ctx->alloc_limit) + " B" : std::string()) + ")");
  }
  *cap = want;
  return DDK_OK;
}

const HostTensor* find_w(ddk_ctx* ctx, const std::string& name, std::initializer_list<int64_t> shape) {
  auto it = ctx->weights.find(name);
  if (it == ctx->weights.end()) { ctx->err = "missing state_dict key: " + name; return nullptr; }
  const std::vector<int64_t> want(shape);
  if (it->second.shape != want) {      // the message names both shapes
    std::string s = "shape mismatch for " + name + ": got [";
    for (auto d : it->second.shape) s += std::to_string(d) + ",";
    s += "] want [";
    for (auto d : want) s += std::to_string(d) + ",";
    ctx->err = s + "]";
    return nullptr;
  }
  return &it->second;
}

int model_finalize(ddk_ctx* ctx);   // model.hip
int conf_model_finalize(ddk_ctx* ctx);   // conf.hip
void conf_model_destroy(ddk_ctx* ctx);
void model_destroy(ddk_ctx* ctx);   // model.hip

}  // namespace ddk

extern "C" {

const char* ddk_version(void) { return "ddk 0.8 (gfx950)"; }      // 0.8: conv_kernel = 0 is the two-limb / three-product form of the f16-limb kernel (k_conv_x2.hip), the three-limb / six-product form (the default of 0.4 - 0.7) is conv_kernel = 3; 0.7: conv_kernel = 2 left the library (the kernel itself was removed later: the last tree carrying it, under tools/variants/, is cd91202), ddk_tp_forward walks columns (flat 16-B reads), ddk_debug_set_alloc_limit; 0.6: conv_kernel = 2 (k_conv_y.hip), streaming ddk_tp_forward, confidence edge capacity from geometry; 0.5: ddk_config.confidence_mode + ddk_score_confidence; 0.4: three-limb records carry limbs at their own weight + tile descriptors; conv_f16x3 removed (INTEGRATION.md "ABI notes")

int ddk_create(const ddk_config* cfg, ddk_ctx** out) {
  if (!cfg || !out) return DDK_ERR_INVALID;
  ddk_ctx* ctx = new ddk_ctx();
  ctx->cfg = *cfg;
  *out = ctx;
  if (cfg->ns != NS || cfg->nv != NV)
    return fail(ctx, DDK_ERR_INVALID, "only ns=24, nv=6 (DiffDock-S / DisCo-DiffDock-S) is compiled in");
  if (cfg->num_conv_layers < 4 || cfg->num_conv_layers > 16)
    return fail(ctx, DDK_ERR_INVALID, "num_conv_layers must be in [4,16] (the heads and the confidence predictor assume the full 0e+1o+1e+0o irreps)");
  if (cfg->confidence_mode && cfg->all_atoms)
    return fail(ctx, DDK_ERR_INVALID, "confidence_mode selects the COARSE-GRAINED score model's confidence head; the all-atom confidence model is all_atoms = 1 alone (include/ddk.h)");
  if (cfg->sigma_embed_dim != 32 || cfg->distance_embed_dim != 32 || cfg->cross_distance_embed_dim != 32)
    return fail(ctx, DDK_ERR_INVALID, "only 32-wide sigma / distance embeddings are compiled in");
  if (cfg->deterministic && cfg->all_atoms)
    return fail(ctx, DDK_ERR_INVALID, "deterministic scatter is implemented for the score model (not with all_atoms)");
  if (cfg->conv_kernel < 0 || cfg->conv_kernel > 3 || cfg->conv_kernel == 2)
    return fail(ctx, DDK_ERR_INVALID, "conv_kernel must be 0 (two f16 limbs per operand, three products), 1 (fp32 MFMA) or 3 (three f16 limbs, six products); 2 (round 5's software-pipelined form) is retired; the last tree that carries it, under tools/variants/, is cd91202");
  if (cfg->device < 0) {
    ctx->host_only = true;   // packing-only context (CPU tests); every launch entry point refuses to run
    return DDK_OK;
  }
  hipError_t e = hipSetDevice(cfg->device);
  if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, cfg->device);
  if (e != hipSuccess) return hip_fail(ctx, e, "hipGetDeviceProperties");
  ctx->n_cu = prop.multiProcessorCount;
  e = hipStreamCreateWithFlags(&ctx->up_stream, hipStreamNonBlocking);
  if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamCreate (upload stream)");
  e = hipStreamCreateWithFlags(&ctx->head_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming);
  if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamCreate (head stream)");
  e = conv_prepare_device();
  if (e != hipSuccess) return hip_fail(ctx, e, "hipFuncSetAttribute(dynamic LDS)");
  e = graph_prepare_device(&ctx->max_rec);
  if (e != hipSuccess) return hip_fail(ctx, e, "hipFuncSetAttribute(dynamic LDS, graph kernels)");
  ctx->ws.tile_info = (int32_t*)dev_alloc(ctx, 64 * sizeof(int32_t));
  if (!ctx->ws.tile_info) return fail(ctx, DDK_ERR_NOMEM, "hipMalloc failed");
  return DDK_OK;
}

void ddk_destroy(ddk_ctx* ctx) {
  if (!ctx) return;
  if (!ctx->host_only) {
    hipSetDevice(ctx->cfg.device);
    model_destroy(ctx);
    conf_model_destroy(ctx);
    for (auto& r : ctx->prof_recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    if (ctx->prof_edges) hipHostFree(ctx->prof_edges);
    for (auto& c : ctx->chunk_pool) { if (c.free_after) hipEventDestroy(c.free_after); ctx_free(ctx, c.p); }
    for (auto& b : ctx->stage_pool) { if (b.done) hipEventDestroy(b.done); hipHostFree(b.p); }
    if (ctx->up_stream) hipStreamDestroy(ctx->up_stream);
    if (ctx->head_stream) hipStreamDestroy(ctx->head_stream);
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
    for (void* p : ctx->dev_allocs) ctx_free(ctx, p);
    if (ctx->ws.xpad) ctx_free(ctx, ctx->ws.xpad);
    if (ctx->ws.sum) ctx_free(ctx, ctx->ws.sum);
    if (ctx->ws.deg) ctx_free(ctx, ctx->ws.deg);
    if (ctx->ws.gumbel_y) ctx_free(ctx, ctx->ws.gumbel_y);
  }
  delete ctx;
}

const char* ddk_last_error(ddk_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ddk_load_weights(ddk_ctx* ctx, const char* name, const float* host_ptr, const int64_t* shape, int32_t ndim) {
  if (!ctx || !name || (!host_ptr && ndim > 0 && shape[0] != 0)) return fail(ctx, DDK_ERR_INVALID, "ddk_load_weights: null argument");
  const std::string n(name);
  if (n.find(".tp.") != std::string::npos) return DDK_OK;   // e3nn-internal buffers of real checkpoints
  HostTensor t;
  int64_t numel = 1;
  for (int i = 0; i < ndim; ++i) {
    t.shape.push_back(shape[i]);
    numel *= shape[i];
  }
  t.data.assign(host_ptr, host_ptr + numel);
  ctx->weights[n] = std::move(t);
  ctx->finalized = false;
  return DDK_OK;
}

int ddk_finalize_weights(ddk_ctx* ctx) {
  if (!ctx) return DDK_ERR_INVALID;
  if (!ctx->host_only) hipSetDevice(ctx->cfg.device);
  ctx->conv.clear();
  ctx->conv.resize(ctx->cfg.num_conv_layers);
  for (int l = 0; l < ctx->cfg.num_conv_layers; ++l) {
    int rc = build_conv_layer(ctx, ctx->cfg.all_atoms ? 1 : 0, l, ctx->conv[l]);
    if (rc != DDK_OK) return rc;
  }
  // the score model's two heads as layouts of the fused conv kernel (also in host-only contexts: the CPU emulation tests read the packing)
  ctx->head[0] = ConvLayerDev(); ctx->head[1] = ConvLayerDev();
  if (!ctx->cfg.all_atoms && ctx->weights.find("final_conv.fc.0.weight") != ctx->weights.end()) {
    int rch = build_head_layer(ctx, 3, ctx->head[1]);
    if (rch == DDK_OK && !ctx->cfg.no_torsion) rch = build_head_layer(ctx, 2, ctx->head[0]);
    if (rch != DDK_OK) return rch;
  }
  int rc = ctx->cfg.all_atoms ? conf_model_finalize(ctx) : model_finalize(ctx);
  if (rc != DDK_OK) return rc;
  ctx->finalized = true;
  return DDK_OK;
}

int ddk_set_score_norm_tables(ddk_ctx* ctx, const double* so3, int32_t n_so3, const double* torus, int32_t n_torus) {
  if (!ctx || !so3 || !torus) return fail(ctx, DDK_ERR_INVALID, "null table");
  if (n_so3 != 1000 || n_torus != 5001) return fail(ctx, DDK_ERR_INVALID, "expected 1000 so3 and 5001 torus entries");
  ctx->so3_table.assign(so3, so3 + n_so3);
  ctx->torus_table.assign(torus, torus + n_torus);
  return DDK_OK;
}

static int check_launchable(ddk_ctx* ctx, int32_t layer) {
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (!ctx->finalized) return fail(ctx, DDK_ERR_STATE, "weights not finalised");
  if (layer < 0 || layer >= (int)ctx->conv.size()) return fail(ctx, DDK_ERR_INVALID, "layer out of range");
  return DDK_OK;
}

// what the six tensor-product entries check first: a context that can launch, and a `layer` that names one of the kernels' shapes: conv layer `layer` of
// the context (ddk_create admits ns = 24, nv = 6 only), or DDK_TP_NV4 + l, layer l of the ns = 24 / nv = 4 family, which no context holds: its
// ConvLayerDev is the static shape-only table of k_tp_shape.h; or, where `aa_ok` (the radial tensor product and the radial conv), DDK_TP_AA + l, layer l of
// the all-atom family (e3nn's FullyConnectedTensorProduct with sh_lmax = 2), a shape-only layer too.  *L: the layer to launch on.  Asked BEFORE the launch, so that an invalid-value error of
// the launch itself is reported as what it is
static const char* const TP_FAMILIES = "0 .. num_conv_layers - 1 of the context (24x0e [+ 6x1o [+ 6x1e [+ 24x0o]]] -> the next entry), DDK_TP_NV4 + 0..4 "
                                       "(24x0e [+ 4x1o [+ 4x1e [+ 24x0o]]] -> the next entry) or, for the radial tensor product and the radial conv, "
                                       "DDK_TP_AA + 0..4 (the all-atom family: the first family's irreps with sh = 1x0e + 1x1o + 1x2e)";
static int check_tp_launchable(ddk_ctx* ctx, const char* who, int32_t layer, const ConvLayerDev** L, bool aa_ok = false) {
  if (tp_is_aa_id(layer)) {
    int rc = check_launchable(ctx, 0);
    if (rc) return rc;
    // the ids name a shape, not a context's layer: a context that holds a conv layer of this index (the all-atom inference context has 45) is refused
    if (layer < (int)ctx->conv.size())
      return fail(ctx, DDK_ERR_INVALID, std::string(who) + ": this context has a conv layer " + std::to_string(layer) + ", and the id is DDK_TP_AA + " +
                  std::to_string(layer - TP_AA) + " of the all-atom family: use a context with at most 16 conv layers for the all-atom shapes");
    if (!aa_ok)
      return fail(ctx, DDK_ERR_INVALID, std::string(who) + ": DDK_TP_AA + " + std::to_string(layer - TP_AA) + " names a shape of the all-atom family, which has no "
                  "per-edge weight form [E, W]: its ops are ddk_rtp_* and ddk_rconv_*");
    *L = &tp_family_layer(layer);
    return DDK_OK;
  }
  if (tp_is_nv4_id(layer)) {
    int rc = check_launchable(ctx, 0);
    if (rc) return rc;
    // a context that holds a conv layer of this index (more than eight layers) ran ITS layer under this id before the second family existed: refused, not reinterpreted
    if (layer < (int)ctx->conv.size())
      return fail(ctx, DDK_ERR_INVALID, std::string(who) + ": this context has a conv layer " + std::to_string(layer) + ", and the id is DDK_TP_NV4 + " +
                  std::to_string(layer - TP_NV4) + " of the nv = 4 family: ask for layer 3, which has the shape of every later layer, or use a context "
                  "with at most eight conv layers for the nv = 4 shapes");
    *L = &tp_family_layer(layer);
    return DDK_OK;
  }
  if (ctx && !ctx->host_only && ctx->finalized && (layer < 0 || layer >= (int)ctx->conv.size()))
    return fail(ctx, DDK_ERR_INVALID, std::string(who) + ": layer out of range: it is " + TP_FAMILIES);
  int rc = check_launchable(ctx, layer);
  if (rc) return rc;
  if (tp_shape_index(ctx->conv[layer]) < 0)
    return fail(ctx, DDK_ERR_INVALID, std::string(who) + ": the layer's irreps are not one of the conv-layer shapes of the two families: " + TP_FAMILIES);
  *L = &ctx->conv[layer];
  return DDK_OK;
}

int ddk_tp_forward(ddk_ctx* ctx, int32_t layer, const float* x_dst, const float* sh, const float* w, int64_t E,
                   float* out, void* stream) {
  const ConvLayerDev* L = nullptr;
  int rc = check_tp_launchable(ctx, "ddk_tp_forward", layer, &L);
  if (rc) return rc;
  hipError_t e = launch_tp_forward(*L, x_dst, sh, w, E, out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "tp_forward launch");
  return DDK_OK;
}

int ddk_tp_backward(ddk_ctx* ctx, int32_t layer, const float* x_dst, const float* sh, const float* w, const float* grad_out, int64_t E,
                    float* grad_x, float* grad_sh, float* grad_w, void* stream) {
  const ConvLayerDev* L = nullptr;
  int rc = check_tp_launchable(ctx, "ddk_tp_backward", layer, &L);
  if (rc) return rc;
  if (!grad_x && !grad_sh && !grad_w) return fail(ctx, DDK_ERR_INVALID, "ddk_tp_backward: no gradient requested (grad_x, grad_sh and grad_w are all null)");
  if (E < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_tp_backward: negative edge count");
  if (E > 0 && (!x_dst || !sh || !grad_out || (!w && (grad_x || grad_sh))))
    return fail(ctx, DDK_ERR_INVALID, "ddk_tp_backward: null operand (w may be null only when grad_w alone is requested)");
  hipError_t e = launch_tp_backward(*L, x_dst, sh, w, grad_out, E, grad_x, grad_sh, grad_w, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "tp_backward launch");
  return DDK_OK;
}

// the group table of a training op and its edge count: 1..4 groups, E below 2^31, a monotone host prefix from 0 to E
static int check_group_table(ddk_ctx* ctx, const char* who, const int64_t* go, int32_t n_groups, int64_t E) {
  const std::string w(who);
  if (n_groups < 1 || n_groups > 4) return fail(ctx, DDK_ERR_INVALID, w + ": n_groups must be in 1..4");
  if (E < 0 || E >= (int64_t)1 << 31) return fail(ctx, DDK_ERR_INVALID, w + ": edge count out of range");
  if (!go) return fail(ctx, DDK_ERR_INVALID, w + ": null group_offsets");
  if (go[0] != 0) return fail(ctx, DDK_ERR_INVALID, w + ": group_offsets must start at 0");
  for (int g = 0; g < n_groups; ++g)
    if (go[g + 1] < go[g]) return fail(ctx, DDK_ERR_INVALID, w + ": group_offsets are not monotone");
  if (go[n_groups] != E) return fail(ctx, DDK_ERR_INVALID, w + ": the last group offset is not E");
  return DDK_OK;
}

// the graph of a conv op (the radial conv, the head convs): node counts below 2^31, and with edges nodes on both sides and the tables the direction reads
static int check_conv_graph(ddk_ctx* ctx, const char* who, const RconvGraph& gr, int64_t E, bool backward) {
  const std::string w(who);
  const int64_t lim = (int64_t)1 << 31;
  if (gr.n_in < 0 || gr.n_in >= lim || gr.n_out < 0 || gr.n_out >= lim) return fail(ctx, DDK_ERR_INVALID, w + ": node count out of range");
  if (E == 0) return DDK_OK;
  if (gr.n_in == 0 || gr.n_out == 0) return fail(ctx, DDK_ERR_INVALID, w + ": edges without nodes");
  if (!gr.src || !gr.dst || !gr.src_order || !gr.src_ptr || (backward && (!gr.dst_order || !gr.dst_ptr)))
    return fail(ctx, DDK_ERR_INVALID, w + ": null graph table (edge_src, edge_dst, the orderings and their pointer tables)");
  return DDK_OK;
}

// the checks the two radial-tensor-product entries share: layer, group table, edge count
static int rtp_check(ddk_ctx* ctx, const char* who, int32_t layer, const int64_t* go, int32_t n_groups, int64_t E, const ConvLayerDev** L) {
  int rc = check_tp_launchable(ctx, who, layer, L, true);
  if (rc) return rc;
  if (layer > 4 && !tp_is_nv4_id(layer) && !tp_is_aa_id(layer))
    return fail(ctx, DDK_ERR_INVALID, std::string(who) + ": layer out of range (0..4, DDK_TP_NV4 + 0..4, or DDK_TP_AA + 0..4 of the all-atom family)");
  return check_group_table(ctx, who, go, n_groups, E);
}

int ddk_rtp_forward(ddk_ctx* ctx, int32_t layer, const float* x_dst, const float* sh, const float* h, const int64_t* group_offsets, int32_t n_groups,
                    const float* w2, const float* b2, int64_t E, float* out, void* stream) {
  const ConvLayerDev* L = nullptr;
  int rc = rtp_check(ctx, "ddk_rtp_forward", layer, group_offsets, n_groups, E, &L);
  if (rc) return rc;
  if (E == 0) return DDK_OK;
  if (!x_dst || !sh || !h || !w2 || !b2 || !out) return fail(ctx, DDK_ERR_INVALID, "ddk_rtp_forward: null operand");
  hipError_t e = launch_rtp_forward(*L, x_dst, sh, h, group_offsets, n_groups, w2, b2, out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "rtp_forward launch");
  return DDK_OK;
}

int ddk_rtp_backward(ddk_ctx* ctx, int32_t layer, const float* x_dst, const float* sh, const float* h, const int64_t* group_offsets, int32_t n_groups,
                     const float* w2, const float* b2, const float* grad_out, int64_t E, float* grad_x, float* grad_sh, float* grad_h, float* grad_w2,
                     float* grad_b2, void* workspace, void* stream) {
  const ConvLayerDev* L = nullptr;
  int rc = rtp_check(ctx, "ddk_rtp_backward", layer, group_offsets, n_groups, E, &L);
  if (rc) return rc;
  if (tp_is_aa_id(layer) && grad_sh)
    return fail(ctx, DDK_ERR_INVALID, "ddk_rtp_backward: grad_sh is not implemented for the all-atom family (DDK_TP_AA ids): pass NULL");
  if (!grad_x && !grad_sh && !grad_h && !grad_w2 && !grad_b2)
    return fail(ctx, DDK_ERR_INVALID, "ddk_rtp_backward: no gradient requested (grad_x, grad_sh, grad_h, grad_w2 and grad_b2 are all null)");
  const bool per_edge = grad_x || grad_sh || grad_h, params = grad_w2 || grad_b2;
  if (E > 0) {
    if (!x_dst || !sh || !h || !grad_out) return fail(ctx, DDK_ERR_INVALID, "ddk_rtp_backward: null operand");
    if (per_edge && !w2) return fail(ctx, DDK_ERR_INVALID, "ddk_rtp_backward: null w2 (it may be null only when grad_x, grad_sh and grad_h are all null)");
    if ((grad_x || grad_sh) && !b2) return fail(ctx, DDK_ERR_INVALID, "ddk_rtp_backward: null b2 (grad_x and grad_sh need w = w2 h + b2)");
    if (params && !workspace) return fail(ctx, DDK_ERR_INVALID, "ddk_rtp_backward: grad_w2 / grad_b2 need the workspace of ddk_rtp_backward_workspace");
  }
  if (E == 0 && !params) return DDK_OK;
  hipError_t e = launch_rtp_backward(*L, x_dst, sh, h, group_offsets, n_groups, w2, b2, grad_out, grad_x, grad_sh, grad_h, grad_w2, grad_b2,
                                     (float*)workspace, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "rtp_backward launch");
  return DDK_OK;
}

int64_t ddk_rtp_backward_workspace(int32_t layer, int64_t E, int32_t n_groups) { return rtp_backward_workspace(layer, E, n_groups); }

// the checks the two radial-conv entries share on top of rtp_check: node counts, and with edges the graph tables and the per-edge operands
static int rconv_check(ddk_ctx* ctx, const char* who, int32_t layer, const int64_t* go, int32_t n_groups, int64_t E, const RconvGraph& gr, bool backward,
                       const float* x_nodes, const float* sh, const float* h, const void* workspace, const ConvLayerDev** L) {
  int rc = rtp_check(ctx, who, layer, go, n_groups, E, L);
  if (!rc) rc = check_conv_graph(ctx, who, gr, E, backward);
  if (rc || E == 0) return rc;
  const std::string w(who);
  if (!x_nodes || !sh || !h) return fail(ctx, DDK_ERR_INVALID, w + ": null operand");
  if (!workspace) return fail(ctx, DDK_ERR_INVALID, w + ": null workspace (ddk_rconv_workspace bytes)");
  return DDK_OK;
}

int ddk_rconv_forward(ddk_ctx* ctx, int32_t layer, const float* x_nodes, int64_t n_in, int64_t n_out, const int32_t* edge_src, const int32_t* edge_dst,
                      const int32_t* src_order, const int64_t* src_ptr, const float* sh, const float* h, const int64_t* group_offsets, int32_t n_groups,
                      const float* w2, const float* b2, int64_t E, float* out_nodes, void* workspace, void* stream) {
  const RconvGraph gr{n_in, n_out, edge_src, edge_dst, src_order, src_ptr, nullptr, nullptr};
  const ConvLayerDev* L = nullptr;
  int rc = rconv_check(ctx, "ddk_rconv_forward", layer, group_offsets, n_groups, E, gr, false, x_nodes, sh, h, workspace, &L);
  if (rc) return rc;
  if (n_out > 0 && !out_nodes) return fail(ctx, DDK_ERR_INVALID, "ddk_rconv_forward: null out_nodes");
  if (E > 0 && (!w2 || !b2)) return fail(ctx, DDK_ERR_INVALID, "ddk_rconv_forward: null w2 or b2");
  hipError_t e = launch_rconv_forward(*L, gr, x_nodes, sh, h, group_offsets, n_groups, w2, b2, out_nodes, (float*)workspace, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "rconv_forward launch");
  return DDK_OK;
}

int ddk_rconv_backward(ddk_ctx* ctx, int32_t layer, const float* x_nodes, int64_t n_in, int64_t n_out, const int32_t* edge_src, const int32_t* edge_dst,
                       const int32_t* src_order, const int64_t* src_ptr, const int32_t* dst_order, const int64_t* dst_ptr, const float* sh, const float* h,
                       const int64_t* group_offsets, int32_t n_groups, const float* w2, const float* b2, const float* grad_out_nodes, int64_t E,
                       float* grad_x_nodes, float* grad_sh, float* grad_h, float* grad_w2, float* grad_b2, void* workspace, void* stream) {
  const RconvGraph gr{n_in, n_out, edge_src, edge_dst, src_order, src_ptr, dst_order, dst_ptr};
  const ConvLayerDev* L = nullptr;
  int rc = rconv_check(ctx, "ddk_rconv_backward", layer, group_offsets, n_groups, E, gr, true, x_nodes, sh, h, workspace, &L);
  if (rc) return rc;
  if (tp_is_aa_id(layer) && grad_sh)
    return fail(ctx, DDK_ERR_INVALID, "ddk_rconv_backward: grad_sh is not implemented for the all-atom family (DDK_TP_AA ids): pass NULL");
  if (!grad_x_nodes && !grad_sh && !grad_h && !grad_w2 && !grad_b2)
    return fail(ctx, DDK_ERR_INVALID, "ddk_rconv_backward: no gradient requested (grad_x_nodes, grad_sh, grad_h, grad_w2 and grad_b2 are all null)");
  if (E > 0) {
    if (!grad_out_nodes) return fail(ctx, DDK_ERR_INVALID, "ddk_rconv_backward: null grad_out_nodes");
    if ((grad_x_nodes || grad_sh || grad_h) && !w2)
      return fail(ctx, DDK_ERR_INVALID, "ddk_rconv_backward: null w2 (it may be null only when grad_x_nodes, grad_sh and grad_h are all null)");
    if ((grad_x_nodes || grad_sh) && !b2) return fail(ctx, DDK_ERR_INVALID, "ddk_rconv_backward: null b2 (grad_x_nodes and grad_sh need w = w2 h + b2)");
  }
  hipError_t e = launch_rconv_backward(*L, gr, x_nodes, sh, h, group_offsets, n_groups, w2, b2, grad_out_nodes, grad_x_nodes, grad_sh, grad_h,
                                       grad_w2, grad_b2, (float*)workspace, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "rconv_backward launch");
  return DDK_OK;
}

int64_t ddk_rconv_workspace(int32_t layer, int64_t E, int32_t n_groups, int64_t n_in, int64_t n_out, int32_t backward) {
  return rconv_workspace(layer, E, n_groups, n_in, n_out, backward);
}

// the checks the two radial-hidden entries share: a context that can launch, the group table, the counts, and with edges the operands both read
static int rhid_check(ddk_ctx* ctx, const char* who, const int64_t* go, int32_t n_groups, int64_t E, int64_t n_nodes, float p, const float* xs,
                      const int32_t* edge_src, const int32_t* edge_dst, const float* emb) {
  int rc = check_launchable(ctx, 0);
  if (rc) return rc;
  const std::string w(who);
  const int64_t lim = (int64_t)1 << 31;
  // (the node count is refused after n_groups and E and before the offsets, as it always was: the refusal tests hold the order)
  if (n_groups >= 1 && n_groups <= 4 && E >= 0 && E < lim && (n_nodes < 0 || n_nodes >= lim)) return fail(ctx, DDK_ERR_INVALID, w + ": node count out of range");
  if ((rc = check_group_table(ctx, who, go, n_groups, E))) return rc;
  if (!(p >= 0.f && p < 1.f)) return fail(ctx, DDK_ERR_INVALID, w + ": the dropout rate p must be in [0, 1)");
  if (E == 0) return DDK_OK;
  if (n_nodes == 0) return fail(ctx, DDK_ERR_INVALID, w + ": edges without nodes");
  if (!xs || !edge_src || !edge_dst || !emb) return fail(ctx, DDK_ERR_INVALID, w + ": null operand (xs, edge_src, edge_dst, emb)");
  if (((uintptr_t)xs | (uintptr_t)emb) & 15) return fail(ctx, DDK_ERR_INVALID, w + ": xs and emb must be 16-byte aligned");
  return DDK_OK;
}

int ddk_rhid_forward(ddk_ctx* ctx, const float* xs, int64_t n_nodes, const int32_t* edge_src, const int32_t* edge_dst, const float* emb,
                     const int64_t* group_offsets, int32_t n_groups, const float* w1, const float* b1, float p, uint64_t seed, int64_t E, float* h,
                     void* stream) {
  int rc = rhid_check(ctx, "ddk_rhid_forward", group_offsets, n_groups, E, n_nodes, p, xs, edge_src, edge_dst, emb);
  if (rc) return rc;
  if (E == 0) return DDK_OK;
  if (!w1 || !b1 || !h) return fail(ctx, DDK_ERR_INVALID, "ddk_rhid_forward: null operand (w1, b1, h)");
  hipError_t e = launch_rhid_forward(xs, edge_src, edge_dst, emb, group_offsets, n_groups, w1, b1, p, seed, h, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "rhid_forward launch");
  return DDK_OK;
}

int ddk_rhid_backward(ddk_ctx* ctx, const float* xs, int64_t n_nodes, const int32_t* edge_src, const int32_t* edge_dst, const int32_t* src_order,
                      const int64_t* src_ptr, const int32_t* dst_order, const int64_t* dst_ptr, const float* emb, const float* h,
                      const int64_t* group_offsets, int32_t n_groups, const float* w1, const float* grad_h, float p, int64_t E, float* grad_xs,
                      float* grad_emb, float* grad_w1, float* grad_b1, void* workspace, void* stream) {
  int rc = rhid_check(ctx, "ddk_rhid_backward", group_offsets, n_groups, E, n_nodes, p, xs, edge_src, edge_dst, emb);
  if (rc) return rc;
  if (!grad_xs && !grad_emb && !grad_w1 && !grad_b1)
    return fail(ctx, DDK_ERR_INVALID, "ddk_rhid_backward: no gradient requested (grad_xs, grad_emb, grad_w1 and grad_b1 are all null)");
  if (E > 0) {
    if (!h || !grad_h) return fail(ctx, DDK_ERR_INVALID, "ddk_rhid_backward: null operand (h, grad_h)");
    if ((grad_xs || grad_emb) && !w1)
      return fail(ctx, DDK_ERR_INVALID, "ddk_rhid_backward: null w1 (it may be null only when grad_xs and grad_emb are both null)");
    if (grad_xs && (!src_order || !src_ptr || !dst_order || !dst_ptr))
      return fail(ctx, DDK_ERR_INVALID, "ddk_rhid_backward: null graph table (grad_xs needs the orderings and their pointer tables)");
    if (!workspace) return fail(ctx, DDK_ERR_INVALID, "ddk_rhid_backward: null workspace (ddk_rhid_workspace bytes)");
    if (((uintptr_t)workspace | (uintptr_t)h | (uintptr_t)grad_h) & 15)
      return fail(ctx, DDK_ERR_INVALID, "ddk_rhid_backward: h, grad_h and the workspace must be 16-byte aligned");
  }
  const RconvGraph gr{n_nodes, n_nodes, edge_src, edge_dst, src_order, src_ptr, dst_order, dst_ptr};
  hipError_t e = launch_rhid_backward(gr, xs, emb, h, group_offsets, n_groups, w1, grad_h, p, grad_xs, grad_emb, grad_w1, grad_b1, (float*)workspace,
                                      (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "rhid_backward launch");
  return DDK_OK;
}

int64_t ddk_rhid_workspace(int64_t E, int32_t n_groups, int64_t n_nodes) { return rhid_workspace(E, n_groups, n_nodes); }

// the checks the two head-conv entries share: a context that can launch, the head, the counts, and with edges the graph tables and the operands both read
static int hconv_check(ddk_ctx* ctx, const char* who, int32_t head, int64_t E, const RconvGraph& gr, bool backward, const float* x_nodes, const float* sh,
                       const float* h, const void* workspace) {
  int rc = check_launchable(ctx, 0);
  if (rc) return rc;
  const std::string w(who);
  if (head != DDK_HEAD_CENTER && head != DDK_HEAD_TORSION) return fail(ctx, DDK_ERR_INVALID, w + ": head must be DDK_HEAD_CENTER or DDK_HEAD_TORSION");
  if (E < 0 || E >= (int64_t)1 << 31) return fail(ctx, DDK_ERR_INVALID, w + ": edge count out of range");
  rc = check_conv_graph(ctx, who, gr, E, backward);
  if (rc || E == 0) return rc;
  if (!x_nodes || !sh || !h) return fail(ctx, DDK_ERR_INVALID, w + ": null operand");
  if (!workspace) return fail(ctx, DDK_ERR_INVALID, w + ": null workspace (ddk_hconv_workspace bytes)");
  if (((uintptr_t)sh | (uintptr_t)h | (uintptr_t)workspace) & 15) return fail(ctx, DDK_ERR_INVALID, w + ": sh, h and the workspace must be 16-byte aligned");
  return DDK_OK;
}

int ddk_hconv_forward(ddk_ctx* ctx, int32_t head, const float* x_nodes, int64_t n_in, int64_t n_out, const int32_t* edge_src, const int32_t* edge_dst,
                      const int32_t* src_order, const int64_t* src_ptr, const float* sh, const float* h, const float* w2, const float* b2, int64_t E,
                      float* out_nodes, void* workspace, void* stream) {
  const RconvGraph gr{n_in, n_out, edge_src, edge_dst, src_order, src_ptr, nullptr, nullptr};
  int rc = hconv_check(ctx, "ddk_hconv_forward", head, E, gr, false, x_nodes, sh, h, workspace);
  if (rc) return rc;
  if (n_out > 0 && !out_nodes) return fail(ctx, DDK_ERR_INVALID, "ddk_hconv_forward: null out_nodes");
  if (E > 0 && (!w2 || !b2)) return fail(ctx, DDK_ERR_INVALID, "ddk_hconv_forward: null w2 or b2");
  hipError_t e = launch_hconv_forward(head, gr, x_nodes, sh, h, w2, b2, E, out_nodes, (float*)workspace, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "hconv_forward launch");
  return DDK_OK;
}

int ddk_hconv_backward(ddk_ctx* ctx, int32_t head, const float* x_nodes, int64_t n_in, int64_t n_out, const int32_t* edge_src, const int32_t* edge_dst,
                       const int32_t* src_order, const int64_t* src_ptr, const int32_t* dst_order, const int64_t* dst_ptr, const float* sh, const float* h,
                       const float* w2, const float* b2, const float* grad_out_nodes, int64_t E, float* grad_x_nodes, float* grad_h, float* grad_w2,
                       float* grad_b2, void* workspace, void* stream) {
  const RconvGraph gr{n_in, n_out, edge_src, edge_dst, src_order, src_ptr, dst_order, dst_ptr};
  int rc = hconv_check(ctx, "ddk_hconv_backward", head, E, gr, true, x_nodes, sh, h, workspace);
  if (rc) return rc;
  if (!grad_x_nodes && !grad_h && !grad_w2 && !grad_b2)
    return fail(ctx, DDK_ERR_INVALID, "ddk_hconv_backward: no gradient requested (grad_x_nodes, grad_h, grad_w2 and grad_b2 are all null)");
  if (E > 0) {
    if (!grad_out_nodes) return fail(ctx, DDK_ERR_INVALID, "ddk_hconv_backward: null grad_out_nodes");
    if ((grad_x_nodes || grad_h) && !w2)
      return fail(ctx, DDK_ERR_INVALID, "ddk_hconv_backward: null w2 (it may be null only when grad_x_nodes and grad_h are both null)");
    if (grad_x_nodes && !b2) return fail(ctx, DDK_ERR_INVALID, "ddk_hconv_backward: null b2 (grad_x_nodes needs w = w2 h + b2)");
  }
  hipError_t e = launch_hconv_backward(head, gr, x_nodes, sh, h, w2, b2, grad_out_nodes, E, grad_x_nodes, grad_h, grad_w2, grad_b2, (float*)workspace,
                                       (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "hconv_backward launch");
  return DDK_OK;
}

int64_t ddk_hconv_workspace(int32_t head, int64_t E, int64_t n_in, int64_t n_out, int32_t backward) { return hconv_workspace(head, E, n_in, n_out, backward); }

// The four edge-embedding entries are two bodies, eemb_forward and eemb_backward: l == nullptr is the plain op, and `who` is the calling entry, whose name
// every message carries.  The checks they share: a context that can launch, the counts and the smearing, and with edges the operands both directions read
static int eemb_check(ddk_ctx* ctx, const char* who, const EembOperands& o, const EembLatent* l, int64_t n_a, int64_t n_b, int64_t n_sig, int32_t n_gauss, int64_t E) {
  int rc = check_launchable(ctx, 0);
  if (rc) return rc;
  const std::string w(who);
  const int64_t lim = (int64_t)1 << 31;
  if (o.F != 0 && o.F != 4) return fail(ctx, DDK_ERR_INVALID, w + ": F must be 0 or 4");
  if (n_gauss != 32) return fail(ctx, DDK_ERR_INVALID, w + ": n_gauss must be 32");
  if (E < 0 || E >= lim) return fail(ctx, DDK_ERR_INVALID, w + ": edge count out of range");
  if (n_a < 0 || n_a >= lim || n_b < 0 || n_b >= lim || n_sig < 0 || n_sig >= lim) return fail(ctx, DDK_ERR_INVALID, w + ": node or graph count out of range");
  if (!(o.p >= 0.f && o.p < 1.f)) return fail(ctx, DDK_ERR_INVALID, w + ": the dropout rate p must be in [0, 1)");
  if (!(o.stop > o.start)) return fail(ctx, DDK_ERR_INVALID, w + ": the smearing needs start < stop");
  if (E > 0) {
    if (n_a == 0 || n_b == 0 || n_sig == 0) return fail(ctx, DDK_ERR_INVALID, w + ": edges without nodes or graphs");
    if (!o.pos_a || !o.pos_b || !o.idx_a || !o.idx_b || !o.sig || !o.sig_index) return fail(ctx, DDK_ERR_INVALID, w + ": null operand (pos, idx, sig, sig_index)");
    if ((o.F == 4) != (o.feat != nullptr)) return fail(ctx, DDK_ERR_INVALID, w + ": feat must be given with F == 4 and null with F == 0");
    if (!o.w1 || !o.b1 || !o.w2) return fail(ctx, DDK_ERR_INVALID, w + ": null parameter (w1, b1, w2)");
    if (((uintptr_t)o.feat | (uintptr_t)o.sig) & 15) return fail(ctx, DDK_ERR_INVALID, w + ": feat and sig must be 16-byte aligned");
  }
  if (!l) return DDK_OK;      // what the two latent entries check on top
  if (l->NL < 1 || l->NL > 4) return fail(ctx, DDK_ERR_INVALID, w + ": L (the latent columns per node) must be in 1..4");
  if (E == 0) return DDK_OK;
  if (!l->zero_latent && (!l->lat_a || !l->lat_b)) return fail(ctx, DDK_ERR_INVALID, w + ": null latent table (lat_a, lat_b; they may be null only with zero_latent)");
  if (!l->zero_latent && (((uintptr_t)l->lat_a | (uintptr_t)l->lat_b) & 15)) return fail(ctx, DDK_ERR_INVALID, w + ": lat_a and lat_b must be 16-byte aligned");
  if (l->unc_a && !l->uemb) return fail(ctx, DDK_ERR_INVALID, w + ": unc_a without uemb");
  return DDK_OK;
}

static int eemb_forward(ddk_ctx* ctx, const char* who, const EembOperands& o, const EembLatent* l, int64_t n_a, int64_t n_b, int64_t n_sig, int32_t n_gauss,
                        int64_t E, float* emb, float* sh, void* stream) {
  int rc = eemb_check(ctx, who, o, l, n_a, n_b, n_sig, n_gauss, E);
  if (rc) return rc;
  if (E == 0) return DDK_OK;
  const std::string w(who);
  if (!o.b2 || !emb || !sh) return fail(ctx, DDK_ERR_INVALID, w + ": null operand (b2, emb, sh)");
  if (((uintptr_t)emb | (uintptr_t)sh) & 15) return fail(ctx, DDK_ERR_INVALID, w + ": emb and sh must be 16-byte aligned");
  hipError_t e = launch_eemb_forward(o, l, E, emb, sh, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, (w.substr(4) + " launch").c_str());      // (the entry's name without "ddk_")
  return DDK_OK;
}

// the plain entry passes null for grad_uemb, grad_lat_a, grad_lat_b and the node-sorted lists of gr
static int eemb_backward(ddk_ctx* ctx, const char* who, const EembOperands& o, const EembLatent* l, const EembLatentGraph& gr, int64_t n_sig, int32_t n_gauss,
                         const float* grad_emb, int64_t E, float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2, float* grad_uemb, float* grad_lat_a,
                         float* grad_lat_b, void* workspace, void* stream) {
  int rc = eemb_check(ctx, who, o, l, gr.n_a, gr.n_b, n_sig, n_gauss, E);
  if (rc) return rc;
  const std::string w(who);
  if (!grad_w1 && !grad_b1 && !grad_w2 && !grad_b2 && !grad_uemb && !grad_lat_a && !grad_lat_b)
    return fail(ctx, DDK_ERR_INVALID, w + (l ? ": no gradient requested (all seven outputs are null)"
                                             : ": no gradient requested (grad_w1, grad_b1, grad_w2 and grad_b2 are all null)"));
  if (E > 0) {
    if (!grad_emb) return fail(ctx, DDK_ERR_INVALID, w + ": null grad_emb");
    if (!workspace) return fail(ctx, DDK_ERR_INVALID, w + ": null workspace (" + (l ? "ddk_eemb_latent_workspace" : "ddk_eemb_workspace") + " bytes)");
    if (((uintptr_t)grad_emb | (uintptr_t)workspace) & 15) return fail(ctx, DDK_ERR_INVALID, w + ": grad_emb and the workspace must be 16-byte aligned");
    if (l && !l->zero_latent && ((grad_lat_a && (!gr.order_a || !gr.ptr_a)) || (grad_lat_b && (!gr.order_b || !gr.ptr_b))))
      return fail(ctx, DDK_ERR_INVALID, w + ": null node-sorted edge list (grad_lat_a needs order_a and ptr_a, grad_lat_b order_b and ptr_b)");
  }
  hipError_t e = launch_eemb_backward(o, l, gr, grad_emb, E, grad_w1, grad_b1, grad_w2, grad_b2, grad_uemb, grad_lat_a, grad_lat_b, (float*)workspace,
                                      (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, (w.substr(4) + " launch").c_str());
  return DDK_OK;
}

int ddk_eemb_forward(ddk_ctx* ctx, const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, const int32_t* idx_a, const int32_t* idx_b,
                     const float* feat, int32_t F, const float* sig, int64_t n_sig, const int32_t* sig_index, float start, float stop, int32_t n_gauss,
                     const float* w1, const float* b1, const float* w2, const float* b2, float p, uint64_t seed, int64_t E, float* emb, float* sh,
                     void* stream) {
  const EembOperands o{pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2, p, seed, F};
  return eemb_forward(ctx, "ddk_eemb_forward", o, nullptr, n_a, n_b, n_sig, n_gauss, E, emb, sh, stream);
}

int ddk_eemb_backward(ddk_ctx* ctx, const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, const int32_t* idx_a, const int32_t* idx_b,
                      const float* feat, int32_t F, const float* sig, int64_t n_sig, const int32_t* sig_index, float start, float stop, int32_t n_gauss,
                      const float* w1, const float* b1, const float* w2, const float* b2, float p, uint64_t seed, const float* grad_emb, int64_t E,
                      float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2, void* workspace, void* stream) {
  const EembOperands o{pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2, p, seed, F};
  const EembLatentGraph gr{n_a, n_b, nullptr, nullptr, nullptr, nullptr};
  return eemb_backward(ctx, "ddk_eemb_backward", o, nullptr, gr, n_sig, n_gauss, grad_emb, E, grad_w1, grad_b1, grad_w2, grad_b2, nullptr, nullptr, nullptr,
                       workspace, stream);
}

int64_t ddk_eemb_workspace(int64_t E, int32_t K) { return eemb_workspace(E, K, 0); }

int ddk_eemb_latent_forward(ddk_ctx* ctx, const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, const int32_t* idx_a, const int32_t* idx_b,
                            const float* feat, int32_t F, const float* sig, int64_t n_sig, const int32_t* sig_index, float start, float stop, int32_t n_gauss,
                            const float* w1, const float* b1, const float* w2, const float* b2, float p, uint64_t seed, const float* lat_a, const float* lat_b,
                            int32_t L, int32_t zero_latent, const float* unc_a, const float* uemb, int64_t E, float* emb, float* sh, void* stream) {
  const EembOperands o{pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2, p, seed, F};
  const EembLatent l{lat_a, lat_b, unc_a, uemb, L, zero_latent != 0};
  return eemb_forward(ctx, "ddk_eemb_latent_forward", o, &l, n_a, n_b, n_sig, n_gauss, E, emb, sh, stream);
}

int ddk_eemb_latent_backward(ddk_ctx* ctx, const float* pos_a, int64_t n_a, const float* pos_b, int64_t n_b, const int32_t* idx_a, const int32_t* idx_b,
                             const float* feat, int32_t F, const float* sig, int64_t n_sig, const int32_t* sig_index, float start, float stop, int32_t n_gauss,
                             const float* w1, const float* b1, const float* w2, const float* b2, float p, uint64_t seed, const float* lat_a, const float* lat_b,
                             int32_t L, int32_t zero_latent, const float* unc_a, const float* uemb, const int32_t* order_a, const int64_t* ptr_a,
                             const int32_t* order_b, const int64_t* ptr_b, const float* grad_emb, int64_t E, float* grad_w1, float* grad_b1, float* grad_w2,
                             float* grad_b2, float* grad_uemb, float* grad_lat_a, float* grad_lat_b, void* workspace, void* stream) {
  const EembOperands o{pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2, p, seed, F};
  const EembLatent l{lat_a, lat_b, unc_a, uemb, L, zero_latent != 0};
  const EembLatentGraph gr{n_a, n_b, order_a, ptr_a, order_b, ptr_b};
  return eemb_backward(ctx, "ddk_eemb_latent_backward", o, &l, gr, n_sig, n_gauss, grad_emb, E, grad_w1, grad_b1, grad_w2, grad_b2, grad_uemb, grad_lat_a,
                       grad_lat_b, workspace, stream);
}

// (the latent entries refuse L = 0, the plain op's layout, like every L outside 1..4)
int64_t ddk_eemb_latent_workspace(int64_t E, int32_t K, int32_t L) { return L < 1 ? -1 : eemb_workspace(E, K, L); }

// The checks every entry over a graph's ligand nodes followed by its receptor nodes shares (RaggedTables).  ``samples``: ddk_gumbel_pick_samples, whose count is
// B samples of one graph, which has no pointer tables and whose rows b n + p must fit 31 bits
static int ragged_check(ddk_ctx* ctx, const char* who, int32_t G, int32_t D, int64_t n_lig, int64_t n_rec, const int64_t* lig_ptr, const int64_t* rec_ptr,
                        bool samples = false) {
  int rc = check_launchable(ctx, 0);
  if (rc) return rc;
  const std::string w(who);
  if (G < 1 || G > 65536) return fail(ctx, DDK_ERR_INVALID, w + (samples ? ": B must be in [1, 65536]" : ": G must be in [1, 65536]"));
  if (D < 1 || D > 4) return fail(ctx, DDK_ERR_INVALID, w + ": D must be in 1..4");
  if (n_lig < 0 || n_rec < 0 || n_lig >= (int64_t)1 << 31 || n_rec >= (int64_t)1 << 31 || (samples && n_lig + n_rec >= (int64_t)1 << 31))
    return fail(ctx, DDK_ERR_INVALID, w + ": node count out of range (n_lig, n_rec in [0, 2^31); for samples of one graph n_lig + n_rec < 2^31)");
  if (!samples && (!lig_ptr || !rec_ptr)) return fail(ctx, DDK_ERR_INVALID, w + ": null lig_ptr or rec_ptr");
  return DDK_OK;
}
// a side that has nodes passes every one of its operands
static int ragged_sides(ddk_ctx* ctx, const char* who, int64_t n_lig, int64_t n_rec, std::initializer_list<const void*> lig, std::initializer_list<const void*> rec,
                        const char* what) {
  bool null = false;
  for (const void* p : lig) null |= n_lig > 0 && !p;
  for (const void* p : rec) null |= n_rec > 0 && !p;
  return null ? fail(ctx, DDK_ERR_INVALID, std::string(who) + ": null operand (" + what + " of a side that has nodes)") : DDK_OK;
}
static int temperature_draw_check(ddk_ctx* ctx, const char* who, float T, int32_t draw) {
  const std::string w(who);
  if (!(T > 0.f) || !(T < INFINITY)) return fail(ctx, DDK_ERR_INVALID, w + ": the temperature must be positive and finite");
  if (draw < 0 || draw >= (1 << 20)) return fail(ctx, DDK_ERR_INVALID, w + ": draw must be in [0, 2^20)");
  return DDK_OK;
}

int ddk_gumbel_softmax_batch(ddk_ctx* ctx, int32_t G, int32_t D, const float* logit_l, int64_t n_lig, const float* logit_r, int64_t n_rec,
                             const int64_t* lig_ptr, const int64_t* rec_ptr, float T, uint64_t seed, const uint64_t* stream_id, int32_t sample, int32_t draw,
                             float* y_l, float* y_r, float* out_l, float* out_r, void* stream) {
  const char* who = "ddk_gumbel_softmax_batch";
  int rc = ragged_check(ctx, who, G, D, n_lig, n_rec, lig_ptr, rec_ptr);
  if (rc || (rc = temperature_draw_check(ctx, who, T, draw))) return rc;
  if (sample < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_gumbel_softmax_batch: sample must be >= 0");
  if (!stream_id) return fail(ctx, DDK_ERR_INVALID, "ddk_gumbel_softmax_batch: null stream_id");
  if ((rc = ragged_sides(ctx, who, n_lig, n_rec, {logit_l, y_l, out_l}, {logit_r, y_r, out_r}, "logit, y, out"))) return rc;
  if (n_lig + n_rec == 0) return DDK_OK;
  hipError_t e = launch_gumbel_forward(RaggedTables{lig_ptr, rec_ptr, n_lig, n_rec, G, D}, T, logit_l, logit_r, seed, stream_id, (uint32_t)sample, (uint32_t)draw,
                                       y_l, y_r, out_l, out_r, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "gumbel_softmax_batch launch");
  return DDK_OK;
}

int ddk_gumbel_pick_samples(ddk_ctx* ctx, int32_t B, int32_t D, const float* logit_l, int64_t n_lig, const float* logit_r, int64_t n_rec, float T, uint64_t seed,
                            uint64_t stream_id, int32_t sample0, int32_t draw, float* lig_latent, float* rec_latent, int32_t* choices, void* stream) {
  const char* who = "ddk_gumbel_pick_samples";
  int rc = ragged_check(ctx, who, B, D, n_lig, n_rec, nullptr, nullptr, true);
  if (rc || (rc = temperature_draw_check(ctx, who, T, draw))) return rc;
  if (sample0 < 0 || (int64_t)sample0 + B - 1 > INT32_MAX) return fail(ctx, DDK_ERR_INVALID, "ddk_gumbel_pick_samples: sample0 must be >= 0 and sample0 + B - 1 < 2^31");
  if ((rc = ragged_sides(ctx, who, n_lig, n_rec, {logit_l, lig_latent}, {logit_r, rec_latent}, "logit, latent"))) return rc;
  if (n_lig + n_rec == 0) return DDK_OK;
  Workspace& ws = ctx->ws;
  if ((rc = ensure(ctx, (void**)&ws.gumbel_y, &ws.gumbel_y_cap, (size_t)B * (size_t)(n_lig + n_rec) * D * sizeof(float)))) return rc;
  hipError_t e = launch_gumbel_pick(B, D, logit_l, n_lig, logit_r, n_rec, T, seed, stream_id, (uint32_t)sample0, (uint32_t)draw, ws.gumbel_y, lig_latent,
                                    rec_latent, choices, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "gumbel_pick_samples launch");
  return DDK_OK;
}

int ddk_gumbel_softmax_batch_backward(ddk_ctx* ctx, int32_t G, int32_t D, const float* y_l, int64_t n_lig, const float* y_r, int64_t n_rec,
                                      const int64_t* lig_ptr, const int64_t* rec_ptr, float T, const float* grad_out_l, const float* grad_out_r,
                                      float* grad_logit_l, float* grad_logit_r, void* stream) {
  const char* who = "ddk_gumbel_softmax_batch_backward";
  int rc = ragged_check(ctx, who, G, D, n_lig, n_rec, lig_ptr, rec_ptr);
  if (rc || (rc = temperature_draw_check(ctx, who, T, 0))) return rc;
  if ((rc = ragged_sides(ctx, who, n_lig, n_rec, {y_l, grad_out_l, grad_logit_l}, {y_r, grad_out_r, grad_logit_r}, "y, grad_out, grad_logit"))) return rc;
  if (n_lig + n_rec == 0) return DDK_OK;
  hipError_t e = launch_gumbel_backward(RaggedTables{lig_ptr, rec_ptr, n_lig, n_rec, G, D}, T, y_l, y_r, grad_out_l, grad_out_r, grad_logit_l, grad_logit_r,
                                        (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "gumbel_softmax_batch_backward launch");
  return DDK_OK;
}

int ddk_rng_latent_keep(ddk_ctx* ctx, uint64_t seed, int32_t n, const uint64_t* stream_id, int32_t sample, int32_t draw, float rate, float* keep_out) {
  if (!ctx) return DDK_ERR_INVALID;
  if (n < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_latent_keep: n must be >= 0");
  if (sample < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_latent_keep: sample must be >= 0");
  if (draw < 0 || draw >= RNG_MAX_STEPS) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_latent_keep: draw must be in [0, " + std::to_string(RNG_MAX_STEPS) + ")");
  if (!(rate >= 0.f && rate <= 1.f)) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_latent_keep: rate must be in [0, 1]");
  if (n > 0 && (!stream_id || !keep_out)) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_latent_keep: null argument");
  for (int32_t i = 0; i < n; ++i) {
    uint32_t w[4];
    rng_block(rng_stream(seed, stream_id[i]), (uint32_t)sample, 12u /* latent keep: DDK_RNG_LAYOUT 1 */, (uint32_t)draw, 0, w);
    keep_out[i] = rng_uniform(w[0]) >= rate ? 1.f : 0.f;
  }
  return DDK_OK;
}

int ddk_rng_decoding_index(ddk_ctx* ctx, uint64_t seed, int32_t n, const uint64_t* stream_id, int32_t sample, int32_t draw, int32_t D, int32_t* idx_out) {
  if (!ctx) return DDK_ERR_INVALID;
  if (n < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_decoding_index: n must be >= 0");
  if (sample < 0) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_decoding_index: sample must be >= 0");
  if (draw < 0 || draw >= RNG_MAX_STEPS) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_decoding_index: draw must be in [0, " + std::to_string(RNG_MAX_STEPS) + ")");
  if (D < 1 || D > 4) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_decoding_index: D must be in 1..4");
  if (n > 0 && (!stream_id || !idx_out)) return fail(ctx, DDK_ERR_INVALID, "ddk_rng_decoding_index: null argument");
  for (int32_t i = 0; i < n; ++i) {
    uint32_t w[4];
    rng_block(rng_stream(seed, stream_id[i]), (uint32_t)sample, 14u /* decoding index: DDK_RNG_LAYOUT 1 */, (uint32_t)draw, 0, w);
    idx_out[i] = (int32_t)(((w[0] >> 8) * (uint32_t)D) >> 24);      // (a 24-bit number times D <= 4 fits 32 bits)
  }
  return DDK_OK;
}

// what the two node cross-entropy entries check on top of ragged_check
static int column_soft_check(ddk_ctx* ctx, const char* who, const int32_t* column, int32_t soft) {
  if (soft != 0 && soft != 1) return fail(ctx, DDK_ERR_INVALID, std::string(who) + ": soft must be 0 or 1");
  if (!column) return fail(ctx, DDK_ERR_INVALID, std::string(who) + ": null column");
  return DDK_OK;
}

int ddk_node_cross_entropy_batch(ddk_ctx* ctx, int32_t G, int32_t D, const float* logit_l, int64_t n_lig, const float* logit_r, int64_t n_rec,
                                 const int64_t* lig_ptr, const int64_t* rec_ptr, const float* teacher_l, const float* teacher_r, const int32_t* column,
                                 int32_t soft, float* loss, int64_t* pick, int64_t* target, double* saved, void* stream) {
  const char* who = "ddk_node_cross_entropy_batch";
  int rc = ragged_check(ctx, who, G, D, n_lig, n_rec, lig_ptr, rec_ptr);
  if (rc || (rc = column_soft_check(ctx, who, column, soft))) return rc;
  if ((rc = ragged_sides(ctx, who, n_lig, n_rec, {logit_l, teacher_l}, {logit_r, teacher_r}, "logit, teacher"))) return rc;
  if (!loss || !pick || !target || !saved) return fail(ctx, DDK_ERR_INVALID, "ddk_node_cross_entropy_batch: null output (loss, pick, target, saved)");
  if (n_lig + n_rec == 0) return DDK_OK;
  const NodeCeArgs a{{lig_ptr, rec_ptr, n_lig, n_rec, G, D}, logit_l, logit_r, teacher_l, teacher_r, column, loss, pick, target, saved, soft};
  hipError_t e = launch_node_ce_forward(a, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "node_cross_entropy_batch launch");
  return DDK_OK;
}

int ddk_node_cross_entropy_batch_backward(ddk_ctx* ctx, int32_t G, int32_t D, const float* logit_l, int64_t n_lig, const float* logit_r, int64_t n_rec,
                                          const int64_t* lig_ptr, const int64_t* rec_ptr, const float* teacher_l, const float* teacher_r,
                                          const int32_t* column, int32_t soft, const float* grad, const int64_t* target, const double* saved,
                                          float* grad_logit_l, float* grad_logit_r, void* stream) {
  const char* who = "ddk_node_cross_entropy_batch_backward";
  int rc = ragged_check(ctx, who, G, D, n_lig, n_rec, lig_ptr, rec_ptr);
  if (rc || (rc = column_soft_check(ctx, who, column, soft))) return rc;
  // (hard mode reads no teacher table)
  if ((rc = ragged_sides(ctx, who, n_lig, n_rec, {logit_l, grad_logit_l, soft ? teacher_l : logit_l}, {logit_r, grad_logit_r, soft ? teacher_r : logit_r},
                         "logit, grad_logit, and with soft = 1 teacher,")))
    return rc;
  if (!grad || !target || !saved) return fail(ctx, DDK_ERR_INVALID, "ddk_node_cross_entropy_batch_backward: null argument (grad, target, saved)");
  if (n_lig + n_rec == 0) return DDK_OK;
  const NodeCeBwdArgs a{{lig_ptr, rec_ptr, n_lig, n_rec, G, D}, logit_l, logit_r, teacher_l, teacher_r, column, grad, target, saved, grad_logit_l, grad_logit_r, soft};
  hipError_t e = launch_node_ce_backward(a, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "node_cross_entropy_batch_backward launch");
  return DDK_OK;
}

int ddk_seg_sum(ddk_ctx* ctx, const float* rows, const int32_t* order, const int64_t* ptr, float* nodes, int64_t n_nodes, int32_t D, void* stream) {
  int rc = check_launchable(ctx, 0);
  if (rc) return rc;
  if (n_nodes < 0 || n_nodes >= (int64_t)1 << 31) return fail(ctx, DDK_ERR_INVALID, "ddk_seg_sum: node count out of range");
  if (D < 1 || D > 128) return fail(ctx, DDK_ERR_INVALID, "ddk_seg_sum: D must be in 1..128");
  if (n_nodes == 0) return DDK_OK;
  if (!rows || !order || !ptr || !nodes) return fail(ctx, DDK_ERR_INVALID, "ddk_seg_sum: null operand");
  hipError_t e = launch_seg_sum(rows, order, ptr, nodes, n_nodes, D, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "seg_sum launch");
  return DDK_OK;
}

int ddk_conv_forward(ddk_ctx* ctx, int32_t layer, const float* x, int64_t N, const int32_t* edge_src,
                     const int32_t* edge_dst, const int64_t* go, const float* edge_attr, const float* sh, float* out,
                     void* stream) {
  // all-atom (confidence) contexts: `layer` is the index of ONE reference conv (conv_layers.{layer}, all_atom_score_model.py:37-50,
  // residual=False): every edge belongs to it, out = BatchNorm(scatter_mean(...))
  const bool aa = ctx && ctx->cfg.all_atoms;
  const int conv_k = aa ? layer % 9 : 0;
  if (aa) layer /= 9;
  int rc = check_launchable(ctx, layer);
  if (rc) return rc;
  if (!go || go[0] != 0 || go[1] < go[0] || go[2] < go[1] || go[3] < go[2] || go[4] < go[3])
    return fail(ctx, DDK_ERR_INVALID, "group_offsets must be a non-decreasing prefix starting at 0");
  if (go[4] >= (int64_t)1 << 31 || N >= (int64_t)1 << 31) return fail(ctx, DDK_ERR_INVALID, "graph too large");      // (edge_src holds int32 node ids)
  hipStream_t s = (hipStream_t)stream;
  const ConvLayerDev& L = ctx->conv[layer];
  if (!L.has_weights) return fail(ctx, DDK_ERR_STATE, "conv layer has no weights loaded");
  Workspace& ws = ctx->ws;
  if ((rc = ensure(ctx, (void**)&ws.xpad, &ws.xpad_cap, (size_t)N * XW * 4))) return rc;
  if ((rc = ensure(ctx, (void**)&ws.sum, &ws.sum_cap, (size_t)N * XW * 4))) return rc;
  if ((rc = ensure(ctx, (void**)&ws.deg, &ws.deg_cap, (size_t)N * 4))) return rc;
  const int64_t E = go[4];
  CK(launch_pad_rows(x, N, L.din, ws.xpad, s), "pad_rows");
  CK(hipMemsetAsync(ws.sum, 0, (size_t)N * XW * 4, s), "memset sum");
  CK(hipMemsetAsync(ws.deg, 0, (size_t)N * 4, s), "memset deg");
  if (E > 0) {
    CK(launch_conv_setup(ws.tile_info, go, s), "conv_setup");
    CK(launch_count_deg(edge_src, E, ws.deg, s), "count_deg");
    ConvLaunch a;
    a.x = ws.xpad; a.src = edge_src; a.dst = edge_dst; a.edge_attr = edge_attr; a.sh = sh; a.sum = ws.sum;
    a.tile_info = ws.tile_info; a.counter = ws.tile_info + 10; a.gather = 0;
    if (aa) {
      CK(launch_conv_one_group(ws.tile_info + 32, 9, conv_k, E, s), "group table");
      a.mode = 1; a.n_groups = 9; a.n_active = 9; a.n_slots = 1; a.slots = 0; a.gbeg = ws.tile_info + 32; a.gend = ws.tile_info + 41;
    }
    CK(launch_conv_fused(L, a, ctx->n_cu, s), "conv_fused");
  }
  // the node stage on rows of dout floats (ws.sum was zeroed above: nothing is cleared behind the read)
  NodeFinalizeArgs FA = {};
  FA.sum = ws.sum; FA.deg = ws.deg; FA.n_lig_total = (int)N; FA.out_stride = L.dout; FA.x_out = out;
  FA.x_in = aa ? nullptr : ws.xpad;      // one conv of an all-atom layer: no residual, its own BatchNorm (conv_k = 0 elsewhere)
  // with no edges the reference returns zeros + residual (tensor_layers.py:149-151): BatchNorm is skipped, dout stays 0
  if (aa || E > 0) { FA.bn_mean = L.bn_mean + conv_k * XW; FA.bn_scale = L.bn_scale + conv_k * XW; FA.bn_bias = L.bn_bias + conv_k * XW; FA.dout = L.dout; }
  CK(launch_node_finalize(FA, s), "node_finalize");
  return DDK_OK;
}

// ---- conformer matching (k_match.hip): the limits both calls and the workspace query share; empty = fine
static std::string match_bad_problem(int32_t n_lig, int32_t n_rot) {
  if (n_lig < 3 || n_lig > MAX_LIG) return "n_lig must be in [3, " + std::to_string(MAX_LIG) + "]";
  if (n_rot < 0 || n_rot > MATCH_MAX_ROT) return "n_rot must be in [0, " + std::to_string(MATCH_MAX_ROT) + "]";
  return "";
}

static std::string match_bad_population(int32_t n_rot, int32_t popsize, int32_t n_islands) {
  if (popsize < 1 || popsize > MATCH_MAX_POPSIZE) return "popsize must be in [1, " + std::to_string(MATCH_MAX_POPSIZE) + "]";
  if (n_islands < 1 || n_islands > MATCH_MAX_ISLANDS) return "n_islands must be in [1, " + std::to_string(MATCH_MAX_ISLANDS) + "]";
  if (match_members(popsize, n_rot) > MATCH_MAX_MEMBERS)
    return "max(5, popsize * n_rot) = " + std::to_string(match_members(popsize, n_rot)) + " members per island, at most " + std::to_string(MATCH_MAX_MEMBERS);
  return "";
}

int64_t ddk_conformer_match_workspace(int32_t n_lig, int32_t n_rot, int32_t popsize, int32_t n_islands) {
  if (!match_bad_problem(n_lig, n_rot).empty() || !match_bad_population(n_rot, popsize, n_islands).empty()) return -1;
  return match_workspace_bytes(n_lig, n_rot, popsize, n_islands);
}

int ddk_conformer_rmsd(ddk_ctx* ctx, int32_t n_lig, const float* pos0, const float* target, const uint8_t* atom_mask, const int32_t* rot_bonds,
                       const uint8_t* mask_rotate, int32_t n_rot, int32_t M, const float* torsions, float* rmsd_out, int32_t* status_out, void* stream) {
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  const std::string bad = match_bad_problem(n_lig, n_rot);
  if (!bad.empty()) return fail(ctx, DDK_ERR_INVALID, "ddk_conformer_rmsd: " + bad);
  if (M < 1 || M > MATCH_MAX_VECTORS) return fail(ctx, DDK_ERR_INVALID, "ddk_conformer_rmsd: M must be in [1, " + std::to_string(MATCH_MAX_VECTORS) + "]");
  if (!pos0 || !target || !rmsd_out || !status_out || (n_rot > 0 && (!rot_bonds || !mask_rotate || !torsions)))
    return fail(ctx, DDK_ERR_INVALID, "ddk_conformer_rmsd: null argument (only atom_mask, and the rotor arrays with n_rot = 0, may be null)");
  const MatchProblem P{n_lig, n_rot, pos0, target, atom_mask, rot_bonds, mask_rotate};
  hipError_t e = launch_conformer_rmsd(P, M, torsions, rmsd_out, status_out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "conformer_rmsd launch");
  return DDK_OK;
}

int ddk_conformer_match(ddk_ctx* ctx, int32_t n_lig, const float* pos0, const float* target, const uint8_t* atom_mask, const int32_t* rot_bonds,
                        const uint8_t* mask_rotate, int32_t n_rot, const ddk_match_options* opt, float* torsions_out, float* pos_out, float* rmsd_out,
                        int32_t* count_out, void* workspace, void* stream) {
  if (!ctx) return DDK_ERR_INVALID;
  if (ctx->host_only) return fail(ctx, DDK_ERR_STATE, "host-only context (device < 0) cannot launch kernels");
  if (!opt) return fail(ctx, DDK_ERR_INVALID, "ddk_conformer_match: null options");
  std::string bad = match_bad_problem(n_lig, n_rot);
  if (bad.empty()) bad = match_bad_population(n_rot, opt->popsize, opt->n_islands);
  if (!bad.empty()) return fail(ctx, DDK_ERR_INVALID, "ddk_conformer_match: " + bad);
  if (opt->maxiter < 0 || opt->maxiter > MATCH_MAX_ITER)
    return fail(ctx, DDK_ERR_INVALID, "ddk_conformer_match: maxiter must be in [0, " + std::to_string(MATCH_MAX_ITER) + "]");
  if (opt->polish_iters < 0 || opt->polish_iters > MATCH_MAX_POLISH)
    return fail(ctx, DDK_ERR_INVALID, "ddk_conformer_match: polish_iters must be in [0, " + std::to_string(MATCH_MAX_POLISH) + "]");
  if (!(opt->tol >= 0.0f)) return fail(ctx, DDK_ERR_INVALID, "ddk_conformer_match: tol must be >= 0");
  if (!pos0 || !target || !pos_out || !rmsd_out || !count_out || !workspace || (n_rot > 0 && (!rot_bonds || !mask_rotate || !torsions_out)))
    return fail(ctx, DDK_ERR_INVALID, "ddk_conformer_match: null argument (only atom_mask, and the rotor arrays with n_rot = 0, may be null)");
  const MatchProblem P{n_lig, n_rot, pos0, target, atom_mask, rot_bonds, mask_rotate};
  const MatchSearch O{opt->popsize, opt->maxiter, opt->polish_iters, opt->n_islands, opt->tol, opt->seed, opt->stream_id};
  hipError_t e = launch_conformer_match(P, O, torsions_out, pos_out, rmsd_out, count_out, workspace, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(ctx, e, "conformer_match launch");
  return DDK_OK;
}

// Test hook: copy a packed host-side array out of the context ("conv.<l>.w2p.<g>", "conv.<l>.units", ...).
// Returns the number of floats (or int32 words) of the item, or a negative status.  buf may be NULL to query.
int64_t ddk_debug_export(ddk_ctx* ctx, const char* what, void* buf, int64_t cap_words) {
  if (!ctx || !what) return DDK_ERR_INVALID;
  int l = 0, g = 0;
  char item[32] = {0};
  const void* src = nullptr;
  int64_t n = 0;
  if (sscanf(what, "conv.%d.%31[a-z0-9_].%d", &l, item, &g) >= 2) {
    const bool head = (l == 100 || l == 101) && ctx->head[l - 100].n_tiles > 0;      // conv.100 = tor_bond_conv, conv.101 = final_conv layouts
    if (!head && (l < 0 || l >= (int)ctx->conv.size())) return fail(ctx, DDK_ERR_INVALID, "bad export index");
    ConvLayerDev& L = head ? ctx->head[l - 100] : ctx->conv[l];
    if (g < 0 || g >= L.n_groups) return fail(ctx, DDK_ERR_INVALID, "bad export index");
    const std::string it(item);
    if (it == "w1p") { src = L.h_w1p[g].data(); n = L.h_w1p[g].size(); }
    else if (it == "b1p") { src = L.h_b1p[g].data(); n = L.h_b1p[g].size(); }
    else if (it == "w2p") { src = L.h_w2p[g].data(); n = L.h_w2p[g].size(); }
    else if (it == "b2p") { src = L.h_b2p[g].data(); n = L.h_b2p[g].size(); }
    else if (it == "wn") { src = L.h_wn.data(); n = L.h_wn.size(); }
    else if (it == "bnp") { src = L.h_bnp.data(); n = L.h_bnp.size(); }
    else if (it == "tiles") { src = L.h_tiles.data(); n = L.h_tiles.size() * (sizeof(TileDesc) / 4); }
    else if (it == "bn_mean") { src = L.h_bn_mean.data(); n = L.h_bn_mean.size(); }
    else if (it == "bn_scale") { src = L.h_bn_scale.data(); n = L.h_bn_scale.size(); }
    else if (it == "bn_bias") { src = L.h_bn_bias.data(); n = L.h_bn_bias.size(); }
    // three-limb f16 kernel: all groups' records (bytes, padded to words) and the power-of-two range scales [w1s[4] | w2s[4]]
    else if (it == "w1x") { src = L.h_w1x.data(); n = L.h_w1x.size() / 4; }
    else if (it == "w2x") { src = L.h_w2x.data(); n = L.h_w2x.size() / 4; }
    else if (it == "w1sx") { src = L.h_w1sx.data(); n = L.h_w1sx.size() / 4; }      // two-limb form: the K = 48 GEMM1 fragments of the node-term split (empty for conv_kernel = 3)
    else if (it == "xscale") { static thread_local float sc[8]; for (int k = 0; k < 4; ++k) { sc[k] = L.w1s[k]; sc[4 + k] = L.w2s[k]; } src = sc; n = 8; }
    else return fail(ctx, DDK_ERR_INVALID, "unknown export item");
  } else {
    return fail(ctx, DDK_ERR_INVALID, "unknown export name");
  }
  if (buf) {
    if (cap_words < n) return fail(ctx, DDK_ERR_INVALID, "export buffer too small");
    memcpy(buf, src, (size_t)n * 4);
  }
  return n;
}

// Test hook: the conv kernel's in-register limb split on a DEVICE array: x [n] is cut into groups of `group` consecutive values, each group is
// range-scaled by its own power of two (like the per-edge scaling of the activations) and split; hi / mid / lo [n] come back as fp32 values
// of the fp16 limbs, scale [n] is the group's power of two:  x * scale == hi + mid 2^-11 + lo 2^-22 exactly (tests/test_gpu_round3.py).
int ddk_debug_split3(ddk_ctx* ctx, const float* x, int64_t n, int32_t group, float* hi, float* mid, float* lo, float* scale, void* stream) {
  if (!ctx || ctx->host_only) return DDK_ERR_STATE;
  if (n < 0 || group < 1 || !x || !hi || !mid || !lo || !scale) return fail(ctx, DDK_ERR_INVALID, "ddk_debug_split3: bad argument");
  hipError_t e = launch_split3_probe(x, n, group, hi, mid, lo, scale, (hipStream_t)stream);
  return e == hipSuccess ? DDK_OK : hip_fail(ctx, e, "split3 probe");
}

}  // extern "C"
