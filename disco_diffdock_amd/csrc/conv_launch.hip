// Host side of the fused conv: the only place that launches a conv kernel, and the small kernels that sit around such a launch.
//
// The three kernel files (k_conv.hip: fp32 MFMA; k_conv_x.hip / k_conv_x2.hip: three / two f16 limbs per fp32 operand) each end in ONE table of their
// instantiations (ConvVariant, k_conv_common.h) and export nothing but its accessor.  Both things a launch needs are derived from those tables here:
// conv_prepare_device opts every entry in to its dynamic LDS, launch_conv_fused looks one entry up by key and launches it through the stored address -
// an instantiation cannot be launched without being opted in.  Which key a (layer, launch) pair maps to, and which pairs are refused, is conv_select.
//
// Around a launch: conv_setup / conv_one_group (group tables of the explicit-boundary entry points), pad_rows, count_deg, the node stage and, in
// deterministic mode, conv_det_fix behind the launch.  The node stage is node_finalize (mean, BatchNorm, residual: the last layer and ddk_conv_forward) or
// node_finalize_pre (the same fused with the next layer's per-node GEMM1 terms); both take their arithmetic from k_node.h and their arguments from one
// block, NodeFinalizeArgs, which is the front of NodePreArgs (ddk_internal.h).
#include "k_conv_common.h"
#include "k_node.h"
#include "model.h"

namespace ddk {

// tile_info[0..4] = prefix of ceil(E_g/32), [5..9] = edge offsets of the groups, [10] = tile counter
__global__ void conv_setup_kernel(int32_t* tile_info, int g0, int g1, int g2, int g3, int g4) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int go[5] = {g0, g1, g2, g3, g4};
    int ts = 0;
    tile_info[0] = 0;
    for (int g = 0; g < 4; ++g) {
      ts += (go[g + 1] - go[g] + 31) / 32;
      tile_info[g + 1] = ts;
    }
    for (int g = 0; g < 5; ++g) tile_info[5 + g] = go[g];
    tile_info[10] = 0;
  }
}

// group table of a single-conv launch (ddk_conv_forward on an all-atom context): gbeg[g] = 0, gend[g] = E for g == k else 0
__global__ void conv_one_group_kernel(int32_t* gt, int n_groups, int k, int E) {
  const int g = threadIdx.x;
  if (g < n_groups) { gt[g] = 0; gt[n_groups + g] = g == k ? E : 0; }
}

__global__ void pad_rows_kernel(const float* x, int64_t n, int din, float* xpad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * XW) return;
  const int64_t r = i / XW;
  const int c = (int)(i % XW);
  xpad[i] = c < din ? x[r * din + c] : 0.0f;
}

__global__ void count_deg_kernel(const int32_t* src, int64_t E, int32_t* deg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < E) atomicAdd(deg + src[i], 1);
}

// scatter 'mean' divisor, e3nn BatchNorm (eval) and the residual of tensor_layers.py:159-166, one thread per output element:
//   out = node_finalize_value(sum, deg, mean, scale, bias) + pad(x_in)
// The parameters are NodeFinalizeArgs' members (launch_node_finalize), n = its n_lig_total + n_rec_total.  rr0_mask is NodePreArgs' member: the plain kernel
// gets none (the masked shared rows belong to a layer 0 that is followed by another layer, which the fused kernel finalizes).
__global__ void node_finalize_kernel(float* sum, const int32_t* deg, const float* x_in, const float* bn_mean,
                                     const float* bn_scale, const float* bn_bias, int64_t n, int dout, int out_stride,
                                     float* out, const float* sum_rr0, int64_t n_lig_total, int n_rec, int clear_sum,
                                     float* zero_extra, int64_t n_extra, int n_slots, const uint8_t* rr0_mask) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (zero_extra != nullptr && i < n_extra) zero_extra[i] = 0.0f;
  if (i >= n * out_stride) return;
  const int64_t r = i / out_stride;
  const int c = (int)(i % out_stride);
  float v = 0.0f;
  if (c < dout) {
    const int d = deg[r];
    float sv = 0.0f;
    for (int sl = 0; sl < n_slots; ++sl) {      // deterministic mode keeps one accumulator per (node, receiving group): added in group order
      sv += sum[(r * n_slots + sl) * XW + c];
      if (clear_sum) sum[(r * n_slots + sl) * XW + c] = 0.0f;
    }
    if (sum_rr0 != nullptr && r >= n_lig_total && !(rr0_mask != nullptr && rr0_mask[r - n_lig_total]))
      sv += sum_rr0[((r - n_lig_total) % n_rec) * XW + c];   // shared layer-0 rec-rec messages
    v = node_finalize_value(sv, d, bn_mean[c], bn_scale[c], bn_bias[c]);
  }
  if (x_in != nullptr && c < XW) v += x_in[r * XW + c];
  out[i] = v;
}

// the kernel around k_node.h's body: MODE 0 the node terms of the rows of x_out; 1: node_finalize of a layer first; 2: the node embedding first
template <int MODE>
__global__ __launch_bounds__(PRE_W) void node_finalize_pre_kernel(NodePreArgs A, NodeEmbedArgs E) {
  node_finalize_pre_body<MODE>(A, E, (int)blockIdx.x, (int)gridDim.x);
}

hipError_t launch_node_finalize_pre(const NodePreArgs& a, bool finalize, hipStream_t s, const NodeEmbedArgs* embed) {
  const int tiles = node_pre_tiles(a);
  if (tiles == 0) return hipSuccess;
  NodeEmbedArgs e = {};
  if (embed) e = *embed;
  if (finalize) hipLaunchKernelGGL(node_finalize_pre_kernel<1>, dim3(tiles), dim3(PRE_W), 0, s, a, e);
  else if (embed) hipLaunchKernelGGL(node_finalize_pre_kernel<2>, dim3(tiles), dim3(PRE_W), 0, s, a, e);
  else hipLaunchKernelGGL(node_finalize_pre_kernel<0>, dim3(tiles), dim3(PRE_W), 0, s, a, e);
  return hipGetLastError();
}

hipError_t launch_conv_setup(int32_t* tile_info, const int64_t* go, hipStream_t s) {
  hipLaunchKernelGGL(conv_setup_kernel, dim3(1), dim3(64), 0, s, tile_info, (int)go[0], (int)go[1], (int)go[2], (int)go[3],
                     (int)go[4]);
  return hipGetLastError();
}

hipError_t launch_conv_one_group(int32_t* gt, int n_groups, int k, int64_t E, hipStream_t s) {
  hipLaunchKernelGGL(conv_one_group_kernel, dim3(1), dim3(64), 0, s, gt, n_groups, k, (int)E);
  return hipGetLastError();
}

hipError_t launch_pad_rows(const float* x, int64_t n, int din, float* xpad, hipStream_t s) {
  const int64_t tot = n * XW;
  if (tot == 0) return hipSuccess;
  hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, x, n, din, xpad);
  return hipGetLastError();
}

hipError_t launch_count_deg(const int32_t* src, int64_t E, int32_t* deg, hipStream_t s) {
  if (E == 0) return hipSuccess;
  hipLaunchKernelGGL(count_deg_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, src, E, deg);
  return hipGetLastError();
}

hipError_t launch_node_finalize(const NodeFinalizeArgs& a, hipStream_t s) {
  const int64_t n = (int64_t)a.n_lig_total + a.n_rec_total;
  int64_t tot = n * a.out_stride;
  if (a.zero_extra != nullptr && a.n_extra > tot) tot = a.n_extra;
  if (tot == 0) return hipSuccess;
  hipLaunchKernelGGL(node_finalize_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a.sum, a.deg, a.x_in, a.bn_mean, a.bn_scale, a.bn_bias, n,
                     a.dout, a.out_stride, a.x_out, a.sum_rr0, (int64_t)a.n_lig_total, a.n_rec, a.clear_sum, a.zero_extra, a.n_extra, a.n_slots,
                     static_cast<const uint8_t*>(nullptr));
  return hipGetLastError();
}

// deterministic mode, after a conv launch: fold the partial rows of every run that straddles 32-edge tiles, in tile order, into the run's
// accumulator row.  One wave per tile; the wave whose tile holds the START of a straddling run walks the chain.
__global__ __launch_bounds__(256) void conv_det_fix_kernel(ConvKArgs A, int dout) {
  const int lane = threadIdx.x & 63;
  int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  int g = 0, gb = 0, ge = 0, bstart = 0;                 // bstart: first 256-edge block of the group (or range) in the launch's work queue
  if (A.det_nr > 0) {                                    // sample-aligned units: tile = (work-queue block, wave) of the conv launch
    const int blk = tile / CONV_WAVES;
    if (blk >= A.det_rng[A.det_nr]) return;
    const DetRange R_ = det_find(A.det_rng, A.det_nr, blk);
    g = R_.g; gb = R_.beg; ge = R_.end; bstart = R_.bstart;
    tile -= bstart * CONV_WAVES;
    if (gb + 32 * tile >= ge) return;
  } else {
    for (; g < A.n_active; ++g) {
      gb = A.gbeg[g]; ge = A.gend[g];
      const int nt = (ge - gb + 31) / 32;
      if (tile < nt) break;
      tile -= nt;
      bstart += (ge - gb + CONV_BLOCK_EDGES - 1) / CONV_BLOCK_EDGES;
    }
    if (g >= A.n_active) return;
  }
  auto prow_of = [&](int t, int which) { return A.part + ((size_t)((bstart + t / CONV_WAVES) * CONV_WAVES + t % CONV_WAVES) * 2 + which) * XW; };
  int e0 = gb + 32 * tile;
  int n = min(32, ge - e0);
  const int s_last = A.src[e0 + n - 1];
  if (!(e0 + n < ge && A.src[e0 + n] == s_last)) return;                         // the last run ends here
  if (A.src[e0] == s_last && e0 > gb && A.src[e0 - 1] == s_last) return;          // ... and did not start here: not the head of its chain
  float acc0 = 0.0f, acc1 = 0.0f;
  const float* prow = prow_of(tile, 1);
  if (lane < dout) acc0 = prow[lane];
  if (lane + 64 < dout) acc1 = prow[lane + 64];
  for (;;) {
    ++tile;
    e0 += 32;
    n = min(32, ge - e0);
    prow = prow_of(tile, 0);
    if (lane < dout) acc0 += prow[lane];
    if (lane + 64 < dout) acc1 += prow[lane + 64];
    if (!(A.src[e0 + n - 1] == s_last && e0 + n < ge && A.src[e0 + n] == s_last)) break;   // the run ends inside this tile
  }
  float* row = (A.sum_g2 != nullptr && g == 2) ? A.sum_g2 + (size_t)(s_last - A.g2_node_off) * XW
                                               : A.sum + ((size_t)s_last * A.n_slots + ((A.slots >> (2 * g)) & 3)) * XW;
  if (lane < dout) row[lane] = acc0;
  if (lane + 64 < dout) row[lane + 64] = acc1;
}

// deterministic mode: the fix-up pass behind a conv launch of any family
static void conv_det_fix(const ConvKArgs& k, const ConvLaunch& a, int dout, hipStream_t s) {
  const int64_t tiles = a.edge_bound / 32 + 8 * CONV_MAX_GROUPS + (int64_t)CONV_WAVES * a.det_nr;      // (every range may end in a partial block)
  hipLaunchKernelGGL(conv_det_fix_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, s, k, dout);
}

// ---- the conv launch ----
enum ConvFamily { CONV_F32, CONV_X3, CONV_X2 };     // k_conv.hip, k_conv_x.hip, k_conv_x2.hip
static ConvTable conv_table(int family) { return family == CONV_F32 ? conv_f32_table() : family == CONV_X3 ? conv_x3_table() : conv_x2_table(); }

// Which kernel a launch runs: (L, a) -> family and key, or hipErrorInvalidValue.
//   family  the layer has limb records (L.w2x) and the launch is mode 0, or mode 1 without node terms (a.pre): the f16 form of L.limbs (2: k_conv_x2, the
//           default; 3: k_conv_x).  Anything else: fp32.
//   key     gather = a.gather, split = gather && a.pre != null (GEMM1 starts from the per-node terms), det = a.part != null, mode = a.mode.
//   fp32    ignores a.trace (a traced forward on a conv_kernel = 1 context runs the plain kernel) and, in mode 1, a.pre (no split kernel there: all 72 inputs);
//           det is refused in a non-zero mode.
//   f16     in this order: the two-limb form refuses split unless the layer has the K = 48 records (L.sender_in_gemm1 && L.w1sx); mode 1 (the confidence model:
//           plain path, atomics) refuses pre, part and trace; det comes before trace - a deterministic launch with a trace pointer runs the DET kernel
//           untraced - and before the epilogue check; the asm-epilogue instantiation (split, not det) is refused unless the tile table has the column shapes it
//           hard-codes (L.epi_ok); trace is the split kernel's and is refused without split.
//   both    det on the gather path needs the split (gather && !pre is refused).
static hipError_t conv_select(const ConvLayerDev& L, const ConvLaunch& a, ConvFamily& family, ConvKey& key) {
  const bool f16 = L.w2x != nullptr && (a.mode == 0 || (a.mode == 1 && a.pre == nullptr));
  family = !f16 ? CONV_F32 : L.limbs == 2 ? CONV_X2 : CONV_X3;
  key.gather = a.gather != 0; key.split = a.gather && a.pre != nullptr; key.det = a.part != nullptr; key.trace = false; key.mode = a.mode == 1 ? 1 : 0;
  if (family == CONV_F32) {
    if (key.det && a.mode != 0) return hipErrorInvalidValue;
    if (key.mode == 1) key.split = false;
  } else {
    if (family == CONV_X2 && key.split && !(L.sender_in_gemm1 && L.w1sx != nullptr)) return hipErrorInvalidValue;
    if (key.mode == 1) {
      if (a.pre != nullptr || a.part != nullptr || a.trace != nullptr) return hipErrorInvalidValue;
    } else if (!key.det) {
      if (key.split && !L.epi_ok) return hipErrorInvalidValue;
      key.trace = a.trace != nullptr;
      if (key.trace && !key.split) return hipErrorInvalidValue;
    }
  }
  if (key.det && key.gather && !key.split) return hipErrorInvalidValue;
  return hipSuccess;
}

// the kernel arguments of a launch: everything but the weights is the same for the three families
static ConvXArgs conv_args(const ConvLayerDev& L, const ConvLaunch& a, bool f16, bool trace) {
  ConvXArgs X = {};
  ConvKArgs& k = X.k;
  k.x = a.x; k.src = a.src; k.dst = a.dst; k.edge_attr = a.edge_attr; k.sh = a.sh; k.sum = a.sum;
  k.counter = a.counter;
  k.b1p = L.b1p[0]; k.n_tiles = L.n_tiles;
  k.n_cols = L.n_cols;
  for (int c = 0; c <= L.n_cols; ++c) k.col_start[c] = L.col_start[c];
  k.sum_g2 = a.sum_g2; k.g2_node_off = a.g2_node_off;
  k.n_groups = a.n_groups; k.n_active = a.n_active; k.n_slots = a.n_slots; k.slots = a.slots; k.wmap = a.wmap;
  if (a.gbeg) { k.gbeg = a.gbeg; k.gend = a.gend; }
  else { k.gbeg = a.tile_info + 5; k.gend = a.tile_info + 6; }   // 4 contiguous groups go[g] .. go[g+1] (explicit-boundary entry point)
  k.pre = a.pre; k.part = a.part; k.det_rng = a.det_rng; k.det_nr = a.det_nr;
  if (f16) {      // the limb records and their power-of-two range scales (w1p / w2r stay null)
    k.w1x = L.w1x; k.w1sx = L.w1sx; k.w2x = L.w2x;
    for (int g = 0; g < CONV_MAX_GROUPS; ++g) { k.w1s[g] = L.w1s[g]; k.w1u[g] = 1.0f / L.w1s[g]; k.w2s[g] = L.w2s[g]; k.w2u[g] = 1.0f / L.w2s[g]; }
  } else {        // the fp32 records (limb pointers stay null, unit scales)
    k.w1p = L.w1p[0]; k.w2r = L.w2r[0];
    for (int g = 0; g < CONV_MAX_GROUPS; ++g) { k.w1s[g] = 1.0f; k.w1u[g] = 1.0f; k.w2s[g] = 1.0f; k.w2u[g] = 1.0f; }
  }
  X.trace = trace ? a.trace : nullptr; X.trace_coarse = a.trace_coarse;
  return X;
}

// opt every conv kernel into > 64 KB of dynamic LDS on the CURRENT device (ddk_create calls this after hipSetDevice: the attribute
// is per device, and a failure is reported by that context instead of being cached for the process)
hipError_t conv_prepare_device() {
  for (int family = CONV_F32; family <= CONV_X2; ++family) {
    const ConvTable t = conv_table(family);
    for (int i = 0; i < t.n; ++i) {
      const hipError_t e = hipFuncSetAttribute(t.v[i].fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.v[i].lds);
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

// one persistent workgroup per CU (its F rows + the W2 ring fill the LDS), dynamic block queue
hipError_t launch_conv_fused(const ConvLayerDev& L, const ConvLaunch& a, int n_cu, hipStream_t s) {
  ConvFamily family;
  ConvKey key;
  hipError_t e = conv_select(L, a, family, key);
  if (e != hipSuccess) return e;
  const ConvTable t = conv_table(family);
  const ConvVariant* v = nullptr;
  for (int i = 0; i < t.n && v == nullptr; ++i) {
    const ConvKey& q = t.v[i].key;
    if (q.gather == key.gather && q.split == key.split && q.det == key.det && q.trace == key.trace && q.mode == key.mode) v = t.v + i;
  }
  if (v == nullptr) return hipErrorInvalidValue;      // (conv_select names no key outside the tables)
  ConvXArgs X = conv_args(L, a, family != CONV_F32, key.trace);
  void* args[] = {family == CONV_F32 ? static_cast<void*>(&X.k) : static_cast<void*>(&X)};      // fp32 kernels take ConvKArgs, f16 kernels ConvXArgs
  (void)hipLaunchKernel(v->fn, dim3(n_cu), dim3(v->threads), args, v->lds, s);
  e = hipGetLastError();
  if (e != hipSuccess || !key.det) return e;
  conv_det_fix(X.k, a, L.dout, s);
  return hipGetLastError();
}

}  // namespace ddk
