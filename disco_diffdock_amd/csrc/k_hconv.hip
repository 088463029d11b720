// The two HEAD convolutions of the score model at the op boundary, and their vector-Jacobian products (include/ddk.h: ddk_hconv_forward / ddk_hconv_backward):
//   out[r] = (1 / max(cnt[r], 1)) sum_{e : src[e] = r, ascending e} TP_head(x[dst[e]], sh[e], W2 h[e] + b2)
// with TP_head e3nn's FullyConnectedTensorProduct of final_conv (head 0, the centre head) or tor_bond_conv (head 1, the torsion head), the per-edge weight
// row w_e = W2 h_e + b2 never stored, forward or backward.  Exact fp32: every sum is an fmaf chain or a sequence of separate multiplies and adds in a fixed
// order (compiled with -ffp-contract=off), no atomics anywhere: the same bits run to run and whichever subset of the gradients is asked for.
//
// THE ARITHMETIC (oracle/e3nn_lite.py: FullyConnectedTensorProduct; conv_pack.hip: build_layout modes 2 and 3).  The node row is x = [a 24 | p 6x3 | q 6x3 | c 24].
//   centre, sh = (s0, v), W = 144, K = 48, out = [2x1o | 2x1e], weights in instruction order, every block [rows][2]:
//     A 0e(x)1o->1o  a v / 6         at 0      B 1o(x)0e->1o  p s0 / 6       at 48     C 1o(x)1o->1e  (p x v) / sqrt72  at 60
//     D 1e(x)0e->1e  q s0 / 6        at 72     E 1e(x)1o->1o  (q x v) / sqrt72  at 84  F 0o(x)1o->1e  c v / 6          at 96
//     (path coefficient sqrt(3/36) times w3j: delta / sqrt3 or epsilon / sqrt6)
//   torsion, sh = (., T) with T the 1o block of the full tensor product, W = 288, K = 72, out = [24x0o | 24x0e], two blocks [6][24]:
//     1o(x)T->0e  (p . T) / sqrt18  at 0, written to columns 24..47          1e(x)T->0o  (q . T) / sqrt18  at 144, written to columns 0..23
//
// TILES.  The weight row is cut into tiles of 36 weights that feed DISJOINT output columns, so the forward needs no exchange between tiles:
//   centre: 4 tiles (o, c) = (parity of the output, its channel): the 24 + 6 + 6 rows of column c of the three blocks that end in that output.  The 1e tiles
//           are the 1o tiles with (a, p, q) read as (c, q, p): one code path, the parity only moves offsets.
//   torsion: 8 tiles (block, 6 output channels): 6 rows x 6 columns.
// A WAVE IS (64 edges, one tile): lane = edge, so a W2 element is the same address for the whole wave and is read through the scalar cache, the edge's h row
// sits in the lane's registers, and w = b2[p] + sum_k W2[p][k] h[k] is one fmaf chain in ascending k.  A workgroup is the NT waves of the same 64 edges (256
// threads for the centre head, 512 for the torsion head); they share the 64 gathered node rows through LDS (stride 85: no bank conflicts).  The grid is
// ceil(E / 64) workgroups: a 1 200-edge centre launch is 76 waves on 19 CUs, a torsion launch of 320 bonds about 800 waves.
//
// LAUNCHES.  Forward: 2 (hc_edge_kernel writes the per-edge rows [E, Dout], seg_kernel<mean> of k_reduce.hip adds a receiver's rows in ascending edge id and divides).
// Backward: at most 4.  hc_edge_kernel<bwd> (grad_x rows and grad_h; the receiver's gradient row is gathered and divided by its count in the kernel),
// seg_kernel of k_reduce.hip (grad_x: a node's rows in ascending edge id), hc_param_kernel + the slice reduction of k_reduce.hip (grad_w2, grad_b2).  Each is skipped when no
// output needs it.
//   backward edge kernel: every wave keeps its tile's part of grad_h (K registers) and of the edge's grad_x row (60 / 18 registers), and the waves add them
//   into one LDS image in tile order, one wave per barrier interval: a fixed order, and the image leaves as coalesced rows.
//   parameter kernel: a workgroup owns (slice of rtp_slice_len(E) edges, tile).  Per 64 staged edges the 36 x 64 values gw = dL/dw_e[p] go to LDS, then every
//   thread adds its (p, k) entries of gw^T [h | 1] over the 64 edges in ascending order.  Partial images [W][K + 1] per slice, added in slice order by
//   slice_reduce_kernel.  The slice length depends on E alone, so the bits do not depend on the device.
// The indices, orderings and pointer tables are trusted: Context.conv_graph (Python) builds and range-checks them.
#include "ddk_internal.h"

namespace ddk {

constexpr int HC_DIN = 84;      // floats of a node row
constexpr int HC_XS = 85;       // LDS stride of a staged node row
constexpr int HC_IS = 65;       // LDS stride of an image column (64 edges)
constexpr int HC_TW = 36;       // weights of a tile
constexpr float HC_S6 = 0.16666666666666666f;        // sqrt(3/36) / sqrt3
constexpr float HC_S72 = 0.11785113019775792f;       // sqrt(3/36) / sqrt6
constexpr float HC_S18 = 0.23570226039551584f;       // sqrt(1/6) / sqrt3

template <int HEAD> struct HcShape;
template <> struct HcShape<0> { static constexpr int W = 144, K = 48, DOUT = 12, NT = 4, GN = 3, NC = 60; };
template <> struct HcShape<1> { static constexpr int W = 288, K = 72, DOUT = 48, NT = 8, GN = 6, NC = 18; };

struct HcArgs {
  const float* x; const float* sh; const float* h; const float* w2; const float* b2; const float* g;      // g: grad_out [n_out, Dout]
  const int32_t* src; const int32_t* dst; const int64_t* src_ptr;
  float* rows;      // forward: the tensor product's rows [E, Dout]
  float* gxr;       // backward: the per-edge rows of grad_x [E, 84], or null
  float* gh; float* ws; float* gw2; float* gb2;
  int64_t E, L;
};

// ---- the centre head's tile (o, c): row rl of 36 = 24 scalar rows, 6 vector rows times s0, 6 vector rows crossed with v ------------------------------------
__device__ __forceinline__ int hc_c_xoff(int o, int rl) {      // the row's first float in the node row
  return rl < 24 ? (o ? 60 : 0) + rl : (rl < 30 ? (o ? 42 : 24) + 3 * (rl - 24) : (o ? 24 : 42) + 3 * (rl - 30));
}
__device__ __forceinline__ int hc_c_wp(int o, int c, int rl) {      // its weight
  return (rl < 24 ? (o ? 96 : 0) + 2 * rl : (rl < 30 ? (o ? 72 : 48) + 2 * (rl - 24) : (o ? 60 : 84) + 2 * (rl - 30))) + c;
}
__device__ __forceinline__ void hc_c_u(int rl, const float* in, float s0, float vx, float vy, float vz, float* u) {      // the pre-weight row, scaled
  if (rl < 24) { const float t = in[0] * HC_S6; u[0] = t * vx; u[1] = t * vy; u[2] = t * vz; }
  else if (rl < 30) { const float t = s0 * HC_S6; u[0] = in[0] * t; u[1] = in[1] * t; u[2] = in[2] * t; }
  else { u[0] = (in[1] * vz - in[2] * vy) * HC_S72; u[1] = (in[2] * vx - in[0] * vz) * HC_S72; u[2] = (in[0] * vy - in[1] * vx) * HC_S72; }
}
// the torsion head's tile (blk, ct): weight i = 6 r + cc of 36
__device__ __forceinline__ int hc_t_wp(int blk, int ct, int r, int cc) { return 144 * blk + 24 * r + 6 * ct + cc; }

template <int HEAD>
__device__ __forceinline__ int hc_wp(int t, int i) {      // weight i of tile t in the weight row
  if constexpr (HEAD == 0) return hc_c_wp(t >> 1, t & 1, i);
  else return hc_t_wp(t >> 2, t & 3, i / 6, i - 6 * (i / 6));
}
template <int HEAD>
__device__ __forceinline__ int hc_out_off(int t) {      // the tile's first column of the output row
  if constexpr (HEAD == 0) return 6 * (t >> 1) + 3 * (t & 1);
  else return ((t >> 2) ? 0 : 24) + 6 * (t & 3);
}

// ---- forward, and the backward's grad_x rows and grad_h -----------------------------------------------------------------------------------------------------
template <int HEAD, bool FWD, bool NX, bool NH>
__global__ __launch_bounds__(64 * HcShape<HEAD>::NT) void hc_edge_kernel(HcArgs a) {
  using S = HcShape<HEAD>;
  constexpr int K = S::K, NTHR = 64 * S::NT;
  constexpr bool G1 = FWD || NX;      // the weights w_e are needed
  __shared__ float xs[64 * HC_XS];
  __shared__ float img[(!FWD && NX) ? HC_DIN * HC_IS : 1];
  __shared__ float ghl[(!FWD && NH) ? K * HC_IS : 1];
  __shared__ int dsts[64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int t = __builtin_amdgcn_readfirstlane(tid >> 6);      // the wave's tile, in a scalar register: W2 and b2 go through the scalar cache
  const int64_t e0 = (int64_t)blockIdx.x * 64, e = e0 + lane;
  const bool ev = e < a.E;
  const int n_e = a.E - e0 < 64 ? (int)(a.E - e0) : 64;
  if (tid < 64) dsts[tid] = ev ? a.dst[e] : 0;
  if constexpr (!FWD && NX) for (int f = tid; f < HC_DIN * HC_IS; f += NTHR) img[f] = 0.f;
  if constexpr (!FWD && NH) for (int f = tid; f < K * HC_IS; f += NTHR) ghl[f] = 0.f;
  __syncthreads();
  for (int f = tid; f < 64 * HC_DIN; f += NTHR) {
    const int r = f / HC_DIN, col = f - r * HC_DIN;
    xs[r * HC_XS + col] = r < n_e ? a.x[(int64_t)dsts[r] * HC_DIN + col] : 0.f;
  }
  float s0 = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
  if (ev) {
    const float4 v = *reinterpret_cast<const float4*>(a.sh + e * 4);
    s0 = v.x; vx = v.y; vy = v.z; vz = v.w;
  }
  float hreg[G1 ? K : 1];
  if constexpr (G1) {
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ev) v = *reinterpret_cast<const float4*>(a.h + e * K + 4 * q);
      hreg[4 * q] = v.x; hreg[4 * q + 1] = v.y; hreg[4 * q + 2] = v.z; hreg[4 * q + 3] = v.w;
    }
  }
  const int ooff = hc_out_off<HEAD>(t);
  float g[FWD ? 1 : S::GN];
  if constexpr (!FWD) {
#pragma unroll
    for (int i = 0; i < S::GN; ++i) g[i] = 0.f;
    if (ev) {
      const int64_t r = a.src[e], cnt = a.src_ptr[r + 1] - a.src_ptr[r];
      const float den = (float)(cnt > 1 ? cnt : 1);
#pragma unroll
      for (int i = 0; i < S::GN; ++i) g[i] = a.g[r * S::DOUT + ooff + i] / den;      // the backward of the mean: a true division, as the forward's
    }
  }
  float o[FWD ? S::GN : 1];
  float gx[(!FWD && NX) ? S::NC : 1];
  float ghr[(!FWD && NH) ? K : 1];
  if constexpr (FWD) {
#pragma unroll
    for (int i = 0; i < S::GN; ++i) o[i] = 0.f;
  }
  if constexpr (!FWD && NH) {
#pragma unroll
    for (int k = 0; k < K; ++k) ghr[k] = 0.f;
  }
  __syncthreads();
  const float* xr = xs + lane * HC_XS;
  if constexpr (HEAD == 0) {
    const int po = t >> 1, pc = t & 1;
#pragma unroll
    for (int rl = 0; rl < HC_TW; ++rl) {
      const int xo = hc_c_xoff(po, rl);
      float in[3], u[3];
      in[0] = xr[xo];
      in[1] = rl >= 24 ? xr[xo + 1] : 0.f;
      in[2] = rl >= 24 ? xr[xo + 2] : 0.f;
      hc_c_u(rl, in, s0, vx, vy, vz, u);
      const int p = hc_c_wp(po, pc, rl);
      const float* wrow = a.w2 + p * K;
      float w = 0.f;
      if constexpr (G1) {
        w = a.b2[p];
#pragma unroll
        for (int k = 0; k < K; ++k) w = fmaf(wrow[k], hreg[k], w);
      }
      if constexpr (FWD) {
        o[0] = fmaf(u[0], w, o[0]); o[1] = fmaf(u[1], w, o[1]); o[2] = fmaf(u[2], w, o[2]);
      }
      if constexpr (!FWD && NX) {
        const float d0 = w * g[0], d1 = w * g[1], d2 = w * g[2];
        if (rl < 24) gx[rl] = (vx * d0 + vy * d1 + vz * d2) * HC_S6;
        else if (rl < 30) { const float ts = s0 * HC_S6; gx[24 + 3 * (rl - 24)] = ts * d0; gx[25 + 3 * (rl - 24)] = ts * d1; gx[26 + 3 * (rl - 24)] = ts * d2; }
        else {
          gx[42 + 3 * (rl - 30)] = (vy * d2 - vz * d1) * HC_S72;
          gx[43 + 3 * (rl - 30)] = (vz * d0 - vx * d2) * HC_S72;
          gx[44 + 3 * (rl - 30)] = (vx * d1 - vy * d0) * HC_S72;
        }
      }
      if constexpr (!FWD && NH) {
        const float gw = u[0] * g[0] + u[1] * g[1] + u[2] * g[2];
#pragma unroll
        for (int k = 0; k < K; ++k) ghr[k] = fmaf(gw, wrow[k], ghr[k]);
      }
    }
  } else {
    const int blk = t >> 2, ct = t & 3;
    const int xb = blk ? 42 : 24;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const float i0 = xr[xb + 3 * r], i1 = xr[xb + 3 * r + 1], i2 = xr[xb + 3 * r + 2];
      const float u = (i0 * vx + i1 * vy + i2 * vz) * HC_S18;
      float du = 0.f;
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) {
        const int p = hc_t_wp(blk, ct, r, cc);
        const float* wrow = a.w2 + p * K;
        float w = 0.f;
        if constexpr (G1) {
          w = a.b2[p];
#pragma unroll
          for (int k = 0; k < K; ++k) w = fmaf(wrow[k], hreg[k], w);
        }
        if constexpr (FWD) o[cc] = fmaf(u, w, o[cc]);
        if constexpr (!FWD && NX) du = fmaf(w, g[cc], du);
        if constexpr (!FWD && NH) {
          const float gw = u * g[cc];
#pragma unroll
          for (int k = 0; k < K; ++k) ghr[k] = fmaf(gw, wrow[k], ghr[k]);
        }
      }
      if constexpr (!FWD && NX) {
        const float ds = du * HC_S18;
        gx[3 * r] = vx * ds; gx[3 * r + 1] = vy * ds; gx[3 * r + 2] = vz * ds;
      }
    }
  }
  if constexpr (FWD) {
    if (ev) {
#pragma unroll
      for (int i = 0; i < S::GN; ++i) a.rows[e * S::DOUT + ooff + i] = o[i];
    }
  } else {
    // the tiles' parts into the workgroup's images, tile after tile: a fixed order of additions
    for (int tt = 0; tt < S::NT; ++tt) {
      if (t == tt) {
        if constexpr (NX) {
          if constexpr (HEAD == 0) {
            const int po = t >> 1;
            const int cs = po ? 60 : 0, cv = po ? 42 : 24, cx = po ? 24 : 42;
#pragma unroll
            for (int i = 0; i < 24; ++i) img[(cs + i) * HC_IS + lane] += gx[i];
#pragma unroll
            for (int i = 0; i < 18; ++i) img[(cv + i) * HC_IS + lane] += gx[24 + i];
#pragma unroll
            for (int i = 0; i < 18; ++i) img[(cx + i) * HC_IS + lane] += gx[42 + i];
          } else {
            const int xb = (t >> 2) ? 42 : 24;
#pragma unroll
            for (int i = 0; i < 18; ++i) img[(xb + i) * HC_IS + lane] += gx[i];
          }
        }
        if constexpr (NH) {
#pragma unroll
          for (int k = 0; k < K; ++k) ghl[k * HC_IS + lane] += ghr[k];
        }
      }
      __syncthreads();
    }
    if constexpr (NX) {
      for (int f = tid; f < n_e * HC_DIN; f += NTHR) {
        const int er = f / HC_DIN, col = f - er * HC_DIN;
        a.gxr[e0 * HC_DIN + f] = img[col * HC_IS + er];
      }
    }
    if constexpr (NH) {
      for (int f = tid; f < n_e * K; f += NTHR) {
        const int er = f / K, col = f - er * K;
        a.gh[e0 * K + f] = ghl[col * HC_IS + er];
      }
    }
  }
}

// ---- parameter gradients ---------------------------------------------------------------------------------------------------------------------------------------
// gw = dL/dw_e[p] of weight i of tile t for one edge: the pre-weight row against the receiver's gradient row gr (not yet divided by the count `den`)
template <int HEAD>
__device__ __forceinline__ float hc_gw(int t, int i, const float* xrow, float s0, float vx, float vy, float vz, const float* gr, float den) {
  if constexpr (HEAD == 0) {
    const int po = t >> 1;
    const int xo = hc_c_xoff(po, i);
    float in[3], u[3];
    in[0] = xrow[xo];
    in[1] = i >= 24 ? xrow[xo + 1] : 0.f;
    in[2] = i >= 24 ? xrow[xo + 2] : 0.f;
    hc_c_u(i, in, s0, vx, vy, vz, u);
    const float* gp = gr + hc_out_off<0>(t);
    return u[0] * (gp[0] / den) + u[1] * (gp[1] / den) + u[2] * (gp[2] / den);
  } else {
    const int r = i / 6, cc = i - 6 * r;
    const float* in = xrow + ((t >> 2) ? 42 : 24) + 3 * r;
    const float u = (in[0] * vx + in[1] * vy + in[2] * vz) * HC_S18;
    return u * (gr[hc_out_off<1>(t) + cc] / den);
  }
}

template <int HEAD>
__global__ __launch_bounds__(256) void hc_param_kernel(HcArgs a) {
  using S = HcShape<HEAD>;
  constexpr int K = S::K, K1 = K + 1, NOUT = HC_TW * K1, NACC = (NOUT + 255) / 256;
  __shared__ float hs[64 * K1];
  __shared__ float gws[HC_TW * 64];
  const int tid = threadIdx.x, t = blockIdx.y;
  const int64_t slice = blockIdx.x, es = slice * a.L, ee = es + a.L < a.E ? es + a.L : a.E;
  float acc[NACC];
#pragma unroll
  for (int n = 0; n < NACC; ++n) acc[n] = 0.f;
  for (int64_t eb = es; eb < ee; eb += 64) {
    const int n_e = ee - eb < 64 ? (int)(ee - eb) : 64;
    __syncthreads();
    for (int f = tid; f < 64 * K1; f += 256) {
      const int r = f / K1, col = f - r * K1;
      hs[f] = r < n_e ? (col < K ? a.h[(eb + r) * K + col] : 1.0f) : 0.f;
    }
    {
      const int el = tid & 63, part = tid >> 6;
      const bool valid = el < n_e;
      const int64_t e = eb + el;
      float s0 = 0.f, vx = 0.f, vy = 0.f, vz = 0.f, den = 1.f;
      const float* xrow = a.x;
      const float* gr = a.g;
      if (valid) {
        const float4 v = *reinterpret_cast<const float4*>(a.sh + e * 4);
        s0 = v.x; vx = v.y; vy = v.z; vz = v.w;
        const int64_t r = a.src[e], cnt = a.src_ptr[r + 1] - a.src_ptr[r];
        den = (float)(cnt > 1 ? cnt : 1);
        xrow = a.x + (int64_t)a.dst[e] * HC_DIN;
        gr = a.g + r * S::DOUT;
      }
      for (int q = 0; q < HC_TW / 4; ++q) {
        const int i = part * (HC_TW / 4) + q;
        gws[i * 64 + el] = valid ? hc_gw<HEAD>(t, i, xrow, s0, vx, vy, vz, gr, den) : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < NACC; ++n) {
      const int idx = tid + 256 * n;
      if (idx < NOUT) {
        const int i = idx / K1, col = idx - i * K1;
        float s = acc[n];
        for (int e2 = 0; e2 < 64; ++e2) s = fmaf(gws[i * 64 + e2], hs[e2 * K1 + col], s);
        acc[n] = s;
      }
    }
  }
  float* image = a.ws + slice * ((int64_t)S::W * K1);
#pragma unroll
  for (int n = 0; n < NACC; ++n) {
    const int idx = tid + 256 * n;
    if (idx < NOUT) {
      const int i = idx / K1, col = idx - i * K1;
      image[hc_wp<HEAD>(t, i) * K1 + col] = acc[n];
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------------------
int64_t hconv_workspace(int32_t head, int64_t E, int64_t n_in, int64_t n_out, int32_t backward) {
  const int64_t lim = (int64_t)1 << 31;
  if (head < 0 || head > 1 || E < 0 || E >= lim || n_in < 0 || n_in >= lim || n_out < 0 || n_out >= lim) return -1;
  const int64_t W = head ? HcShape<1>::W : HcShape<0>::W, K1 = (head ? HcShape<1>::K : HcShape<0>::K) + 1, dout = head ? HcShape<1>::DOUT : HcShape<0>::DOUT;
  if (!backward) return ws_pad(E * dout) * (int64_t)sizeof(float);      // the tensor product's rows
  return (ws_pad(E * HC_DIN) + slice_bound(E, 1) * W * K1) * (int64_t)sizeof(float);      // the per-edge rows of grad_x, the parameter images
}

static HcArgs hc_args(const RconvGraph& gr, const float* x, const float* sh, const float* h, const float* w2, const float* b2, int64_t E) {
  HcArgs a{};
  a.x = x; a.sh = sh; a.h = h; a.w2 = w2; a.b2 = b2;
  a.src = gr.src; a.dst = gr.dst; a.src_ptr = gr.src_ptr;
  a.E = E; a.L = rtp_slice_len(E);
  return a;
}

template <int HEAD>
static hipError_t hc_forward(const RconvGraph& gr, HcArgs a, float* out_nodes, float* workspace, hipStream_t s) {
  using S = HcShape<HEAD>;
  if (a.E == 0) return zero_async(out_nodes, gr.n_out * S::DOUT, s);
  a.rows = workspace;
  const int64_t nwg = (a.E + 63) / 64;      // E < 2^31
  hipLaunchKernelGGL((hc_edge_kernel<HEAD, true, false, false>), dim3((unsigned)nwg), dim3(64 * S::NT), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_seg_mean(workspace, gr.src_order, gr.src_ptr, out_nodes, gr.n_out, S::DOUT, s);
}

template <int HEAD>
static hipError_t hc_backward(const RconvGraph& gr, HcArgs a, float* grad_x_nodes, float* workspace, hipStream_t s) {
  using S = HcShape<HEAD>;
  if (a.E == 0) {
    hipError_t e = zero_async(grad_x_nodes, gr.n_in * HC_DIN, s);
    if (e == hipSuccess) e = zero_async(a.gw2, (int64_t)S::W * S::K, s);
    if (e == hipSuccess) e = zero_async(a.gb2, S::W, s);
    return e;
  }
  float* gx_rows = workspace;
  a.gxr = grad_x_nodes ? gx_rows : nullptr;
  a.ws = gx_rows + ws_pad(a.E * HC_DIN);
  const int64_t nwg = (a.E + 63) / 64;
  const dim3 b(64 * S::NT);
  const bool nx = a.gxr != nullptr, nh = a.gh != nullptr;
  if (nx || nh) {
    if (nx && nh) hipLaunchKernelGGL((hc_edge_kernel<HEAD, false, true, true>), dim3((unsigned)nwg), b, 0, s, a);
    else if (nx) hipLaunchKernelGGL((hc_edge_kernel<HEAD, false, true, false>), dim3((unsigned)nwg), b, 0, s, a);
    else hipLaunchKernelGGL((hc_edge_kernel<HEAD, false, false, true>), dim3((unsigned)nwg), b, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (nx) {
      e = launch_seg_sum(gx_rows, gr.dst_order, gr.dst_ptr, grad_x_nodes, gr.n_in, HC_DIN, s);
      if (e != hipSuccess) return e;
    }
  }
  if (a.gw2 || a.gb2) {
    const int64_t nsl = (a.E + a.L - 1) / a.L;      // at most 241
    hipLaunchKernelGGL((hc_param_kernel<HEAD>), dim3((unsigned)nsl, S::NT), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_slice_reduce(a.ws, group_table(a.E), a.L, ReducePart{a.gw2, a.gb2, S::W, S::K}, ReducePart{}, s);
  }
  return hipGetLastError();
}

hipError_t launch_hconv_forward(int head, const RconvGraph& gr, const float* x_nodes, const float* sh, const float* h, const float* w2, const float* b2, int64_t E,
                                float* out_nodes, float* workspace, hipStream_t s) {
  const HcArgs a = hc_args(gr, x_nodes, sh, h, w2, b2, E);
  return head ? hc_forward<1>(gr, a, out_nodes, workspace, s) : hc_forward<0>(gr, a, out_nodes, workspace, s);
}

hipError_t launch_hconv_backward(int head, const RconvGraph& gr, const float* x_nodes, const float* sh, const float* h, const float* w2, const float* b2,
                                 const float* grad_out_nodes, int64_t E, float* grad_x_nodes, float* grad_h, float* grad_w2, float* grad_b2, float* workspace,
                                 hipStream_t s) {
  HcArgs a = hc_args(gr, x_nodes, sh, h, w2, b2, E);
  a.g = grad_out_nodes; a.gh = grad_h; a.gw2 = grad_w2; a.gb2 = grad_b2;
  return head ? hc_backward<1>(gr, a, grad_x_nodes, workspace, s) : hc_backward<0>(gr, a, grad_x_nodes, workspace, s);
}

}  // namespace ddk
