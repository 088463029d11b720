// The "radial tensor product" of a conv layer at the op boundary, and its vector-Jacobian product, WITHOUT the per-edge weight tensor [E, W]:
//   w_e = W2[g(e)] h_e + b2[g(e)]  (never stored)      out_e = FasterTensorProduct(x_e, sh_e, w_e)      (models/tensor_layers.py:65-116, 154-156)
// From grad_out the VJP gives grad_x, grad_sh (as k_tp_bwd.hip, w_e recomputed), grad_h = gw_e W2, grad_w2[g] = sum_e gw_e (x) h_e and grad_b2[g] = sum_e gw_e,
// where gw_e[k, r, c] = rs_k U_k[r] . g_k[c] (tests/tp_backward_ref.py) is never stored either.  Exact fp32: every GEMM runs on v_mfma_f32_32x32x2_f32
// (bitwise an fmaf chain), no atomics anywhere, the same bits run to run and whichever subset of the outputs is asked for (compiled with -ffp-contract=off).
//
// TILES.  The weight row is cut into tiles of 32 SLOTS = 4 rows x 8 columns of one weight block; slot i of a tile is row 4 rg + ((i>>2)&1) + 2 (i>>4) and
// column 8 cg + (i&3) + 4 ((i>>3)&1).  A scalar block (24 columns) has 3 column groups, a vector block (nv = 6 or 4 columns) one with two or four idle columns; rows past the
// block's end are idle slots (zero operands).  Layer 3: 24 + 9 + 9 + 24 = 66 tiles for 58.5 tiles' worth of weights.  The slot order is chosen for the
// accumulator map of the MFMA (row = (reg&3) + 8 (reg>>2) + 4 (lane>>5)): in EVERY tile a lane's 16 registers hold the same 8 columns, known at compile time,
// and two rows (4 rg + (lane>>5) and that + 2), so the contraction with U or g indexes registers statically and needs two rows of U per lane and tile.
//
// ORIENTATION of the w_tile contraction: EDGES ALONG THE ACCUMULATOR'S LANES (column j = lane & 31 is the edge, the 16 registers are weight slots), the out / G
// row of the edge in the lane's registers.  The other choice (weight columns along lanes) needs a reduction over the rows of a block across lanes for every
// tile; here the only exchange between lanes is one add of the two half-waves at the end of a block (they hold different rows of the same edge).  It also makes
// the lane the owner of its edge's x, sh, g rows: U rows are made on the fly from the edge's node row (no U table, unlike k_tp_bwd.hip: 36 rows x 32 edges x
// 3 would not fit four waves' LDS).
//
// rtp_edge_kernel (forward, and backward pass 2: grad_x, grad_sh, grad_h).  A workgroup is four waves = 4 x 32 edges of ONE group; the waves share each W2
// tile through LDS (one load from L2 per 128 edges: 16 FLOP per byte of W2 would be the L2's ceiling with one wave), once in the A-fragment order of
// GEMM 1 (w_tile = W2_tile H^T, K = 72 walked as k = 36 (lane>>5) + s: 36 MFMAs; the bias initialises the accumulators) and, for grad_h, once row-major as
// the B operand of GEMM 2 (grad_h += gw_tile W2_tile: K = the tile's 32 slots, N = 72 padded to 96: 48 MFMAs into three persistent accumulators; rows
// 4 apart are 288 floats = 32 banks apart, so the two half-waves do not meet).  gw_tile is made on the VALU, one element per lane and step.  G rows are
// folded into grad_x (an LDS image [Din][32] per wave) and grad_sh (registers) as soon as their three column groups are done.
//
// rtp_param_kernel (backward pass 3) + the slice reduction of k_reduce.hip.  A workgroup owns (edge slice of a group, four tiles): wave w keeps the [32 slots x 96] accumulators
// of its tile over the whole slice, gw_tile^T . [h | 1] with K = edges (32 staged in LDS per step; lane = slot makes its gw from the staged x, sh, g rows);
// column 72, against ones, is grad_b2.  Each workgroup stores its partial image [W][73] with plain stores; the second kernel adds the slices of a group in
// slice order.  The slice length depends on E alone (rtp_slice_len: 512 edges, longer once E > 122 880 so that there are never more than 240 + G slices:
// at most 133 MB of workspace for W = 1872), so the bits do not depend on the device.
//
// THE RADIAL CONV (launch_rconv_forward / launch_rconv_backward: node rows to aggregated node rows, lines 153-159 of TensorProductConvLayer.forward).  The same
// two kernels instantiated on RtpIdx<shape>: x and g are node tables, the lane (edge kernel) or the staging loop (parameter kernel) reads row xi[e] = edge_dst[e]
// of x and row gi[e] = edge_src[e] of g; sh, h and all output rows stay per edge.  Around them seg_kernel of k_reduce.hip adds a node's rows in ascending edge id from a
// node-sorted edge list, one thread per (node, column): the scatter-mean of the forward ([E, Dout] rows over src) and the backward of the gather ([E, Din]
// rows of grad_x over dst); rtp_node_scale_kernel makes gn = grad_out / max(count, 1) once per node, so that the backward gathers plain rows.  No atomics
// here either.  The indices, orderings and pointer tables are trusted: Context.conv_graph (Python) builds and range-checks them.
//
// THE ALL-ATOM FAMILY (S::AA, k_tp_shape.h: the confidence model's conv layers, e3nn's FullyConnectedTensorProduct with sh_lmax = 2).  The same two kernels:
// sh rows have 9 floats, blocks 1 and 2 end in the rows of the kind RTP_V2 (vector (x) Y2 -> vector), a slot's place in the weight row is e3nn's
// (S::WROW), and there is no grad_sh.  Everything the family adds stands under `if constexpr (S::AA)`, so the other shapes compile to what they were.
#include <stdlib.h>

#include "ddk_internal.h"
#include "k_tp_shape.h"

namespace ddk {

typedef float rtp_f16 __attribute__((ext_vector_type(16)));
#define RTP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

constexpr int RTP_H = 72;            // width of the radial MLP's hidden layer (3 ns)
constexpr int RTP_EPB = 128;         // edges per workgroup of rtp_edge_kernel
constexpr int RTP_IMG = RTP_H + 1;   // columns of a partial image: grad_w2's 72 and grad_b2

struct RtpArgs {
  const float* x; const float* sh; const float* h; const float* w2; const float* b2; const float* g;
  float* out; float* gx; float* gsh; float* gh; float* ws; float* gw2; float* gb2;
  EdgeGroupTable t;
  int64_t L;      // edges per slice (pass 3)
  const int32_t* xi; const int32_t* gi;      // the indexed kernels (the radial conv): edge e reads row xi[e] of x and row gi[e] of g
};

template <class S>
struct RtpT {      // the tiles of a shape: row groups and column groups of block k, its first tile, the number of tiles
  static constexpr int NRG(int k) { return S::O(k) ? (S::R(k) + 3) / 4 : 0; }
  static constexpr int NCG(int k) { return S::vec(k) ? 1 : 3; }
  static constexpr int T0(int k) { return k <= 0 ? 0 : T0(k - 1) + NRG(k - 1) * NCG(k - 1); }
  static constexpr int NT = T0(4);
  static_assert(S::O0 == 24 && (S::O3 == 0 || S::O3 == 24) && S::O1 <= 8 && S::O2 <= 8, "three column groups of 8, or one of up to 8 (nv = 6: two idle columns, nv = 4: four)");
};

struct RtpSlot { int blk, r, c, p; bool valid; };

template <class S>
__device__ __forceinline__ RtpSlot rtp_slot(int T, int i) {      // slot i of tile T (tiles in the order block, row group, column group)
  using TT = RtpT<S>;
  RtpSlot s;
  s.blk = T < TT::T0(1) ? 0 : (T < TT::T0(2) ? 1 : (T < TT::T0(3) ? 2 : 3));
  const int tt = T - (s.blk == 0 ? 0 : (s.blk == 1 ? TT::T0(1) : (s.blk == 2 ? TT::T0(2) : TT::T0(3))));
  const int ncg = (s.blk == 1 || s.blk == 2) ? 1 : 3;
  const int Ok = s.blk == 0 ? S::O0 : (s.blk == 1 ? S::O1 : (s.blk == 2 ? S::O2 : S::O3));
  const int Rk = s.blk == 0 ? S::R0 : (s.blk == 1 ? S::R1 : (s.blk == 2 ? S::R2 : S::R3));
  const int Bk = s.blk == 0 ? S::B0 : (s.blk == 1 ? S::B1 : (s.blk == 2 ? S::B2 : S::B3));
  const int rg = tt / ncg, cg = tt - rg * ncg;
  s.r = 4 * rg + ((i >> 2) & 1) + 2 * (i >> 4);
  s.c = 8 * cg + (i & 3) + 4 * ((i >> 3) & 1);
  s.valid = s.r < Rk && s.c < Ok;
  if constexpr (S::AA) s.p = s.valid ? S::WROW(s.blk, s.r) + s.c : 0;      // e3nn's instruction order: a compile-time table of the shape
  else s.p = s.valid ? Bk + s.r * Ok + s.c : 0;
  return s;
}

// what makes row r of block k: the kind of product and where its input sits in the node row
enum { RTP_SS = 0, RTP_SV = 1, RTP_VS = 2, RTP_VX = 3, RTP_VD = 4, RTP_NONE = 5, RTP_V2 = 6 };      // scalar s0, scalar (x) v, vector s0, (vector x v)/sqrt2, (vector . v)/sqrt3; all-atom family: sqrt(3/10) M(Y2) vector
struct RtpRow { int kind, xoff, xstep; };

template <class S>
__device__ __forceinline__ RtpRow rtp_row(int k, int r) {
  constexpr int A = S::A, P = S::P, Q = S::Q, C = S::C, XP = S::A, XQ = S::A + 3 * S::P, XC = S::XC;
  RtpRow o{RTP_NONE, 0, 0};
  if (k == 0) {
    if (r < A) o = RtpRow{RTP_SS, r, 0};
    else if (r < A + P) o = RtpRow{RTP_VD, XP + 3 * (r - A), 1};
  } else if (k == 1) {
    if (r < A) o = RtpRow{RTP_SV, r, 0};
    else if (r < A + P) o = RtpRow{RTP_VS, XP + 3 * (r - A), 1};
    else if (r < A + P + Q) o = RtpRow{RTP_VX, XQ + 3 * (r - A - P), 1};
    else if (S::AA && r < A + P + Q + P) o = RtpRow{RTP_V2, XP + 3 * (r - A - P - Q), 1};      // 1o (x) 2e -> 1o
  } else if (k == 2) {
    if (r < P) o = RtpRow{RTP_VX, XP + 3 * r, 1};
    else if (r < P + Q) o = RtpRow{RTP_VS, XQ + 3 * (r - P), 1};
    else if (r < P + Q + C) o = RtpRow{RTP_SV, XC + (r - P - Q), 0};
    else if (S::AA && r < P + Q + C + Q) o = RtpRow{RTP_V2, XQ + 3 * (r - P - Q - C), 1};      // 1e (x) 2e -> 1e
  } else {
    if (r < Q) o = RtpRow{RTP_VD, XQ + 3 * r, 1};
    else if (r < Q + C) o = RtpRow{RTP_SS, XC + (r - Q), 0};
  }
  return o;
}

template <class S>
__device__ __forceinline__ float rtp_rs(int k) {      // of a block index that is a run-time value (the chain is written out: k_tp_shape.h)
  const int Rk = k == 0 ? S::R0 : (k == 1 ? S::R1 : (k == 2 ? S::R2 : S::R3));
  return TP_RS(Rk);
}

// row of U times rs (scalar blocks: u[0] alone)
__device__ __forceinline__ void rtp_u(int kind, const float* i, float s0, float vx, float vy, float vz, float rs, float* u) {
  u[0] = 0.f; u[1] = 0.f; u[2] = 0.f;
  if (kind == RTP_SS) { u[0] = i[0] * s0; }
  else if (kind == RTP_SV) { u[0] = i[0] * vx; u[1] = i[0] * vy; u[2] = i[0] * vz; }
  else if (kind == RTP_VS) { u[0] = i[0] * s0; u[1] = i[1] * s0; u[2] = i[2] * s0; }
  else if (kind == RTP_VX) { u[0] = (i[1] * vz - i[2] * vy) * TP_INV_S2; u[1] = (i[2] * vx - i[0] * vz) * TP_INV_S2; u[2] = (i[0] * vy - i[1] * vx) * TP_INV_S2; }
  else if (kind == RTP_VD) { u[0] = (i[0] * vx + i[1] * vy + i[2] * vz) * TP_INV_S3; }
  u[0] *= rs; u[1] *= rs; u[2] *= rs;
}

// The all-atom family's row kind, vector (x) Y2 -> vector: u = rs sqrt(3/10) M i, with M the symmetric traceless matrix of the five Y2 components
// y = sh[4..8] (e3nn's order: xz, xy, y^2 - (x^2 + z^2)/2, yz, (z^2 - x^2)/2, each times its normalisation) that w3j(1, 2, 1) defines:
//   M = [[-y2/sqrt3 - y4, y1, y0], [y1, 2 y2/sqrt3, y3], [y0, y3, -y2/sqrt3 + y4]].
// M is its own adjoint, so the same product with c = 1 folds a G row into grad_x (rtp_fold_aa)
__device__ __forceinline__ void rtp_m2(const float* y, const float* i, float c, float* u) {
  const float d = y[2] * TP_INV_S3;
  u[0] = ((y[1] * i[1] + y[0] * i[2]) - (d + y[4]) * i[0]) * c;
  u[1] = ((y[1] * i[0] + y[3] * i[2]) + (d + d) * i[1]) * c;
  u[2] = ((y[0] * i[0] + y[3] * i[1]) + (y[4] - d) * i[2]) * c;
}

// the adjoint of rtp_u without rs: a G row (scalar blocks: G[0]) into the edge's grad_x image (stride 32 floats per column) and grad_sh
__device__ __forceinline__ void rtp_fold(const RtpRow& rk, const float* i, const float* G, float s0, float vx, float vy, float vz, float* gxl, bool want_gx, float* gs) {
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  if (rk.kind == RTP_SS) { d0 = s0 * G[0]; gs[0] += i[0] * G[0]; }
  else if (rk.kind == RTP_SV) { d0 = vx * G[0] + vy * G[1] + vz * G[2]; gs[1] += i[0] * G[0]; gs[2] += i[0] * G[1]; gs[3] += i[0] * G[2]; }
  else if (rk.kind == RTP_VS) { d0 = s0 * G[0]; d1 = s0 * G[1]; d2 = s0 * G[2]; gs[0] += i[0] * G[0] + i[1] * G[1] + i[2] * G[2]; }
  else if (rk.kind == RTP_VX) {
    d0 = (vy * G[2] - vz * G[1]) * TP_INV_S2; d1 = (vz * G[0] - vx * G[2]) * TP_INV_S2; d2 = (vx * G[1] - vy * G[0]) * TP_INV_S2;
    gs[1] += (G[1] * i[2] - G[2] * i[1]) * TP_INV_S2; gs[2] += (G[2] * i[0] - G[0] * i[2]) * TP_INV_S2; gs[3] += (G[0] * i[1] - G[1] * i[0]) * TP_INV_S2;
  } else if (rk.kind == RTP_VD) {
    const float k3 = G[0] * TP_INV_S3;
    d0 = vx * k3; d1 = vy * k3; d2 = vz * k3;
    gs[1] += i[0] * k3; gs[2] += i[1] * k3; gs[3] += i[2] * k3;
  }
  if (want_gx && rk.kind != RTP_NONE) {
    gxl[32 * rk.xoff] += d0;
    if (rk.xstep) { gxl[32 * (rk.xoff + 1)] += d1; gxl[32 * (rk.xoff + 2)] += d2; }
  }
}

// rtp_u of the all-atom family (y: the edge's Y2 components, rs = sqrt(1 / R_k): with the constants of rtp_u and TP_S3_10 a path's scale is e3nn's
// sqrt(dim_out / R_k) times the Frobenius-normalised w3j)
__device__ __forceinline__ void rtp_u_aa(int kind, const float* i, float s0, float vx, float vy, float vz, const float* y, float rs, float* u) {
  rtp_u(kind, i, s0, vx, vy, vz, rs, u);
  if (kind == RTP_V2) rtp_m2(y, i, TP_S3_10 * rs, u);
}

// rtp_fold of the all-atom family: grad_x alone (grad_sh is not implemented for it: poses are data where it trains)
__device__ __forceinline__ void rtp_fold_aa(const RtpRow& rk, const float* i, const float* G, float s0, float vx, float vy, float vz, const float* y, float* gxl) {
  float d[3] = {0.f, 0.f, 0.f};
  if (rk.kind == RTP_SS) { d[0] = s0 * G[0]; }
  else if (rk.kind == RTP_SV) { d[0] = vx * G[0] + vy * G[1] + vz * G[2]; }
  else if (rk.kind == RTP_VS) { d[0] = s0 * G[0]; d[1] = s0 * G[1]; d[2] = s0 * G[2]; }
  else if (rk.kind == RTP_VX) { d[0] = (vy * G[2] - vz * G[1]) * TP_INV_S2; d[1] = (vz * G[0] - vx * G[2]) * TP_INV_S2; d[2] = (vx * G[1] - vy * G[0]) * TP_INV_S2; }
  else if (rk.kind == RTP_VD) { const float k3 = G[0] * TP_INV_S3; d[0] = vx * k3; d[1] = vy * k3; d[2] = vz * k3; }
  else if (rk.kind == RTP_V2) { rtp_m2(y, G, TP_S3_10, d); }
  if (rk.kind != RTP_NONE) {
    gxl[32 * rk.xoff] += d[0];
    if (rk.xstep) { gxl[32 * (rk.xoff + 1)] += d[1]; gxl[32 * (rk.xoff + 2)] += d[2]; }
  }
}

// ---- forward and backward pass 2 ---------------------------------------------------------------------------------------------------------------------------
// The compile-time flag IDX of the edge and parameter kernels, carried by the shape type so that the kernels of the plain shapes keep their symbols and
// their code: with S = RtpIdx<shape>, x and g are NODE tables and edge e reads rows a.xi[e] / a.gi[e] of them (the radial conv); sh, h and every output row
// stay per edge
template <class S> struct RtpIdx : S {};
template <class S> struct RtpIsIdx { static constexpr bool value = false; };
template <class S> struct RtpIsIdx<RtpIdx<S>> { static constexpr bool value = true; };

template <bool AA> struct RtpY2 {};                         // the lane's Y2 components: the all-atom family alone holds them
template <> struct RtpY2<true> { float y2[5]; };

template <class S, bool FWD, bool NX, bool NH>
struct RtpEdge : RtpY2<S::AA> {
  using TT = RtpT<S>;
  static constexpr bool IDX = RtpIsIdx<S>::value;
  static constexpr bool G1 = FWD || NX;      // GEMM 1 (w_tile) runs

  const RtpArgs& a;
  float4* Afrag; float* Wrm; float* Bt; float* gxl;      // LDS: the tile as GEMM 1's A fragments, row-major, its bias; this lane's column of the wave's grad_x image
  const float* w2g; const float* b2g;
  int tid, lane, j, hh;
  int64_t e; bool ev, wave_on;
  int64_t ex, eg;      // IDX: the lane's rows of x and g
  float hreg[G1 ? 36 : 1];
  float s0, vx, vy, vz;
  rtp_f16 accH[NH ? 3 : 1];
  float gs[4];
  float4 pre[3]; float preb;
  int T;

  __device__ __forceinline__ RtpEdge(const RtpArgs& a_) : a(a_) {}
  __device__ __forceinline__ int64_t xrow() const { if constexpr (IDX) return ex; else return e; }
  __device__ __forceinline__ int64_t grow() const { if constexpr (IDX) return eg; else return e; }

  __device__ __forceinline__ void fetch(int Tn) {      // global -> registers
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int f = tid + 256 * n;
      pre[n] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f < 576) {
        const int q4 = f >> 6, l = f & 63;
        const RtpSlot s = rtp_slot<S>(Tn, l & 31);
        if (s.valid) {
          const tp_f4 q = *reinterpret_cast<const tp_f4*>(w2g + (int64_t)s.p * RTP_H + 36 * (l >> 5) + 4 * q4);
          pre[n] = make_float4(q.x, q.y, q.z, q.w);
        }
      }
    }
    preb = 0.f;
    if (G1 && tid < 32) {
      const RtpSlot s = rtp_slot<S>(Tn, tid);
      if (s.valid) preb = b2g[s.p];
    }
  }
  __device__ __forceinline__ void park() {      // registers -> LDS
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int f = tid + 256 * n;
      if (f < 576) {
        const int q4 = f >> 6, l = f & 63;
        if (G1) Afrag[f] = pre[n];
        if (NH) reinterpret_cast<float4*>(Wrm)[(l & 31) * 18 + 9 * (l >> 5) + q4] = pre[n];
      }
    }
    if (G1 && tid < 32) Bt[tid] = preb;
  }

  template <int K>
  __device__ __forceinline__ void block() {
    constexpr int Ok = S::O(K), Rk = S::R(K), NCG = TT::NCG(K), NRG = TT::NRG(K);
    constexpr bool VEC = S::vec(K);
    constexpr int NO = VEC ? 3 * Ok : Ok;      // floats of the block in an out / grad_out row
    const float rs = rtp_rs<S>(K);
    float o[FWD && NO > 0 ? NO : 1];
    float gr[FWD || NO == 0 ? 1 : NO];
    if constexpr (FWD) {
#pragma unroll
      for (int c = 0; c < NO; ++c) o[c] = 0.f;
    } else {
#pragma unroll
      for (int c = 0; c < NO; ++c) gr[c] = ev ? a.g[grow() * S::DOUT + S::OUT_OFF(K) + c] : 0.f;
    }
    for (int rg = 0; rg < NRG; ++rg) {
      // the lane's two rows of the tile
      RtpRow rk[2];
      float in[2][3], u[2][3], G[2][3];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int r = 4 * rg + hh + 2 * m;
        rk[m] = r < Rk ? rtp_row<S>(K, r) : RtpRow{RTP_NONE, 0, 0};
#pragma unroll
        for (int k = 0; k < 3; ++k) in[m][k] = (ev && rk[m].kind != RTP_NONE) ? a.x[xrow() * S::DIN + rk[m].xoff + k * rk[m].xstep] : 0.f;
        if constexpr (S::AA) { if constexpr (FWD || NH) rtp_u_aa(rk[m].kind, in[m], s0, vx, vy, vz, this->y2, rs, u[m]); }
        else if constexpr (FWD || NH) rtp_u(rk[m].kind, in[m], s0, vx, vy, vz, rs, u[m]);
        G[m][0] = 0.f; G[m][1] = 0.f; G[m][2] = 0.f;
      }
#pragma unroll
      for (int cg = 0; cg < NCG; ++cg) {
        const bool more = T + 1 < TT::NT;
        if (more) fetch(T + 1);
        if (wave_on) {
          rtp_f16 acc;
          if constexpr (G1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float4 bq = reinterpret_cast<const float4*>(Bt)[2 * q + hh];
              acc[4 * q] = bq.x; acc[4 * q + 1] = bq.y; acc[4 * q + 2] = bq.z; acc[4 * q + 3] = bq.w;
            }
#pragma unroll
            for (int q4 = 0; q4 < 9; ++q4) {
              const float4 av = Afrag[q4 * 64 + lane];
              acc = RTP_MFMA(av.x, hreg[4 * q4], acc);
              acc = RTP_MFMA(av.y, hreg[4 * q4 + 1], acc);
              acc = RTP_MFMA(av.z, hreg[4 * q4 + 2], acc);
              acc = RTP_MFMA(av.w, hreg[4 * q4 + 3], acc);
            }
          }
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const int cl = (t & 3) + 4 * ((t >> 2) & 1), m = t >> 3;
            if (VEC && cl >= Ok) continue;
            const int c = 8 * cg + cl;
            if constexpr (FWD) {
              if constexpr (VEC) { o[3 * c] += u[m][0] * acc[t]; o[3 * c + 1] += u[m][1] * acc[t]; o[3 * c + 2] += u[m][2] * acc[t]; }
              else o[c] += u[m][0] * acc[t];
            }
            if constexpr (NX) {
              if constexpr (VEC) { G[m][0] += acc[t] * gr[3 * c]; G[m][1] += acc[t] * gr[3 * c + 1]; G[m][2] += acc[t] * gr[3 * c + 2]; }
              else G[m][0] += acc[t] * gr[c];
            }
          }
          if constexpr (NH) {
#pragma unroll
            for (int s = 0; s < 16; ++s) {
              const int cl = (s & 3) + 4 * ((s >> 2) & 1), m = s >> 3, c = 8 * cg + cl;
              float gw = 0.f;
              if constexpr (VEC) { if (cl < Ok) gw = u[m][0] * gr[3 * c] + u[m][1] * gr[3 * c + 1] + u[m][2] * gr[3 * c + 2]; } else gw = u[m][0] * gr[c];
              const int brow = (s & 3) + 8 * (s >> 2) + 4 * hh;
#pragma unroll
              for (int n = 0; n < 3; ++n) {
                const float bv = (n < 2 || j < RTP_H - 64) ? Wrm[brow * RTP_H + 32 * n + j] : 0.f;
                accH[n] = RTP_MFMA(gw, bv, accH[n]);
              }
            }
          }
        }
        __syncthreads();
        if (more) park();
        __syncthreads();
        ++T;
      }
      if constexpr (NX) if (wave_on) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          G[m][0] *= rs; G[m][1] *= rs; G[m][2] *= rs;
          if constexpr (S::AA) rtp_fold_aa(rk[m], in[m], G[m], s0, vx, vy, vz, this->y2, gxl);
          else rtp_fold(rk[m], in[m], G[m], s0, vx, vy, vz, gxl, a.gx != nullptr, gs);
        }
      }
    }
    if constexpr (FWD) if (wave_on) {
#pragma unroll
      for (int c = 0; c < NO; ++c) {
        const float tot = o[c] + __shfl_xor(o[c], 32);
        if (ev && (c & 1) == hh) a.out[e * S::DOUT + S::OUT_OFF(K) + c] = tot;
      }
    }
  }

  __device__ __forceinline__ void run(float4* Afrag_, float* Wrm_, float* Bt_, float* gx_img) {
    Afrag = Afrag_; Wrm = Wrm_; Bt = Bt_;
    tid = threadIdx.x; lane = tid & 63; j = lane & 31; hh = lane >> 5;
    const int wave = tid >> 6;
    // the workgroup's group and its first edge: groups in order, ceil(n / 128) workgroups each.  (group_unit written out with the GROUP's end for ge: with
    // the unit's end the backward instantiation for grad_x and grad_h, at 256 vector registers, takes two more accumulation registers)
    int grp = -1;
    int64_t gb = 0, ge = 0, b = blockIdx.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < a.t.n_groups && grp < 0) {
        const int64_t nb = (a.t.off[q + 1] - a.t.off[q] + RTP_EPB - 1) / RTP_EPB;
        if (b < nb) { grp = q; gb = a.t.off[q]; ge = a.t.off[q + 1]; } else b -= nb;
      }
    }
    if (grp < 0) return;
    const int64_t e0 = gb + b * RTP_EPB + 32 * wave;
    wave_on = e0 < ge;
    e = e0 + j;
    ev = e < ge;
    w2g = a.w2 + (int64_t)grp * S::W * RTP_H;
    b2g = G1 ? a.b2 + (int64_t)grp * S::W : nullptr;
    if (G1) {
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        tp_f4 v;
        v.x = 0.f; v.y = 0.f; v.z = 0.f; v.w = 0.f;
        if (ev) v = *reinterpret_cast<const tp_f4*>(a.h + e * RTP_H + 36 * hh + 4 * q);
        hreg[4 * q] = v.x; hreg[4 * q + 1] = v.y; hreg[4 * q + 2] = v.z; hreg[4 * q + 3] = v.w;
      }
    }
    s0 = 0.f; vx = 0.f; vy = 0.f; vz = 0.f;
    if constexpr (S::AA) {      // rows of 9 floats: [Y0 | Y1 | Y2]
#pragma unroll
      for (int k = 0; k < 5; ++k) this->y2[k] = ev ? a.sh[e * 9 + 4 + k] : 0.f;
      if (ev) { s0 = a.sh[e * 9]; vx = a.sh[e * 9 + 1]; vy = a.sh[e * 9 + 2]; vz = a.sh[e * 9 + 3]; }
    } else if (ev) {
      const tp_f4 v = *reinterpret_cast<const tp_f4*>(a.sh + e * 4);
      s0 = v.x; vx = v.y; vy = v.z; vz = v.w;
    }
    if constexpr (IDX) {
      ex = 0; eg = 0;
      if (ev) {
        ex = a.xi[e];
        if (!FWD) eg = a.gi[e];
      }
    }
    gs[0] = 0.f; gs[1] = 0.f; gs[2] = 0.f; gs[3] = 0.f;
    float* img = gx_img + wave * (S::DIN * 32);
    gxl = img + j;
    if (NX) {
      for (int f = lane; f < S::DIN * 32; f += 64) img[f] = 0.f;
    }
    if (NH) {
#pragma unroll
      for (int n = 0; n < 3; ++n)
#pragma unroll
        for (int t = 0; t < 16; ++t) accH[n][t] = 0.f;
    }
    T = 0;
    fetch(0);
    park();
    __syncthreads();
    block<0>();
    if constexpr (S::O(1) > 0) block<1>();
    if constexpr (S::O(2) > 0) block<2>();
    if constexpr (S::O(3) > 0) block<3>();
    if (NH && wave_on) {
      // D of GEMM 2: column = lane & 31 (hidden unit 32 n + j), row = edge (t & 3) + 8 (t >> 2) + 4 (lane >> 5) of the wave's 32
#pragma unroll
      for (int n = 0; n < 3; ++n) {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int64_t er = e0 + (t & 3) + 8 * (t >> 2) + 4 * hh;
          if (er < ge && 32 * n + j < RTP_H) a.gh[er * RTP_H + 32 * n + j] = accH[n][t];
        }
      }
    }
    if (NX) {
      if (a.gsh) {
        float tot[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[k] = gs[k] + __shfl_xor(gs[k], 32);
        if (ev && hh == 0) {
          tp_f4 v;
          v.x = tot[0]; v.y = tot[1]; v.z = tot[2]; v.w = tot[3];
          *reinterpret_cast<tp_f4*>(a.gsh + e * 4) = v;
        }
      }
      __syncthreads();
      if (a.gx && wave_on) {
        const int64_t left = ge - e0;
        const int n_e = left < 32 ? (int)left : 32;
        for (int f = lane; f < n_e * S::DIN; f += 64) {
          const int er = f / S::DIN, col = f - er * S::DIN;
          a.gx[e0 * S::DIN + f] = img[32 * col + er];
        }
      }
    }
  }
};

template <class S, bool FWD, bool NX, bool NH>
__global__ __launch_bounds__(256) void rtp_edge_kernel(RtpArgs a) {
  __shared__ float4 Afrag[(FWD || NX) ? 576 : 1];
  __shared__ float4 Wrm4[NH ? 576 : 1];
  __shared__ float4 Bt4[8];
  __shared__ float gx_img[NX ? 4 * S::DIN * 32 : 1];
  RtpEdge<S, FWD, NX, NH> k(a);
  k.run(Afrag, reinterpret_cast<float*>(Wrm4), reinterpret_cast<float*>(Bt4), gx_img);
}

// ---- backward pass 3: parameter gradients --------------------------------------------------------------------------------------------------------------------
template <class S>
__global__ __launch_bounds__(256) void rtp_param_kernel(RtpArgs a) {
  using TT = RtpT<S>;
  constexpr bool IDX = RtpIsIdx<S>::value;
  constexpr int NCH = (TT::NT + 3) / 4;
  __shared__ float xs[32 * S::DIN];
  __shared__ float gsm[32 * S::DOUT];
  __shared__ float hs[32 * RTP_H];
  __shared__ float4 shs4[32];
  float* shs = reinterpret_cast<float*>(shs4);
  [[maybe_unused]] float* shy = nullptr;      // the all-atom family: the staged edges' Y2 components, [32][5] (shs4 keeps [Y0 | Y1])
  if constexpr (S::AA) {
    __shared__ float shy_buf[32 * 5];
    shy = shy_buf;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hh = lane >> 5;
  const int chunk = blockIdx.x % NCH;
  const int64_t slice = blockIdx.x / NCH;
  const GroupUnit un = group_unit(a.t, slice, a.L);      // the slice's group and edges
  if (un.grp < 0) return;
  const int64_t es = un.begin, ee = un.end;
  const int T = 4 * chunk + wave;
  const bool active = T < TT::NT;
  const RtpSlot sl = rtp_slot<S>(active ? T : 0, j);
  const bool vec = S::vec(sl.blk);
  const RtpRow rk = (active && sl.valid) ? rtp_row<S>(sl.blk, sl.r) : RtpRow{RTP_NONE, 0, 0};
  const int goff = S::OUT_OFF(sl.blk) + (sl.valid ? (vec ? 3 * sl.c : sl.c) : 0);
  const int gstep = (vec && sl.valid) ? 1 : 0;
  const float rs = rtp_rs<S>(sl.blk);
  rtp_f16 acc[3];
#pragma unroll
  for (int n = 0; n < 3; ++n)
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[n][t] = 0.f;
  // IDX: the rows of x (entries 0..31) and g (32..63) of the 32 staged edges, loaded one step ahead into two alternating LDS buffers, so that the staging
  // loops below issue one global load per element, as without the index
  [[maybe_unused]] int* idx_s = nullptr;
  [[maybe_unused]] int step = 0;
  if constexpr (IDX) {
    __shared__ int idx_buf[128];
    idx_s = idx_buf;
    if (tid < 64) {
      const int64_t en = es + (tid & 31);
      idx_s[tid] = en < ee ? (tid < 32 ? a.xi[en] : a.gi[en]) : 0;
    }
  }
  for (int64_t eb = es; eb < ee; eb += 32) {
    const int n_e = ee - eb < 32 ? (int)(ee - eb) : 32;
    __syncthreads();
    if constexpr (IDX) {      // row f / DIN of the 32 staged edges comes from the node table
      const int* cur = idx_s + 64 * (step & 1);
      for (int f = tid; f < 32 * S::DIN; f += 256) {
        const int r = f / S::DIN;
        xs[f] = r < n_e ? a.x[(int64_t)cur[r] * S::DIN + (f - r * S::DIN)] : 0.f;
      }
      for (int f = tid; f < 32 * S::DOUT; f += 256) {
        const int r = f / S::DOUT;
        gsm[f] = r < n_e ? a.g[(int64_t)cur[32 + r] * S::DOUT + (f - r * S::DOUT)] : 0.f;
      }
      ++step;
      if (tid < 64) {      // the next step's rows, visible after the barrier below; the buffer they go to was last read before the barrier above
        const int64_t en = eb + 32 + (tid & 31);
        idx_s[64 * (step & 1) + tid] = en < ee ? (tid < 32 ? a.xi[en] : a.gi[en]) : 0;
      }
    } else {
      for (int f = tid; f < 32 * S::DIN; f += 256) xs[f] = f < n_e * S::DIN ? a.x[eb * S::DIN + f] : 0.f;
      for (int f = tid; f < 32 * S::DOUT; f += 256) gsm[f] = f < n_e * S::DOUT ? a.g[eb * S::DOUT + f] : 0.f;
    }
    for (int f = tid; f < 32 * RTP_H; f += 256) hs[f] = f < n_e * RTP_H ? a.h[eb * RTP_H + f] : 0.f;
    if constexpr (S::AA) {
      for (int f = tid; f < 32 * 9; f += 256) {
        const int r = f / 9, k = f - 9 * r;
        const float v = r < n_e ? a.sh[eb * 9 + f] : 0.f;
        if (k < 4) shs[4 * r + k] = v; else shy[5 * r + k - 4] = v;
      }
    } else if (tid < 128) shs[tid] = tid < n_e * 4 ? a.sh[eb * 4 + tid] : 0.f;
    __syncthreads();
    if (active) {
#pragma unroll 4
      for (int s = 0; s < 16; ++s) {
        const int el = 16 * hh + s;      // K index (lane >> 5, s) is edge 16 (lane >> 5) + s of the 32
        float in[3], u[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) in[k] = xs[el * S::DIN + rk.xoff + k * rk.xstep];
        const float4 sv = shs4[el];
        if constexpr (S::AA) rtp_u_aa(rk.kind, in, sv.x, sv.y, sv.z, sv.w, shy + 5 * el, rs, u);
        else rtp_u(rk.kind, in, sv.x, sv.y, sv.z, sv.w, rs, u);
        const float g0 = gsm[el * S::DOUT + goff], g1 = gsm[el * S::DOUT + goff + gstep], g2 = gsm[el * S::DOUT + goff + 2 * gstep];
        const float gw = vec ? u[0] * g0 + u[1] * g1 + u[2] * g2 : u[0] * g0;
#pragma unroll
        for (int n = 0; n < 3; ++n) {
          const int col = 32 * n + j;
          const float bv = col < RTP_H ? hs[el * RTP_H + col] : (col == RTP_H ? 1.0f : 0.f);
          acc[n] = RTP_MFMA(gw, bv, acc[n]);
        }
      }
    }
  }
  if (active) {
    float* img = a.ws + slice * ((int64_t)S::W * RTP_IMG);
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const RtpSlot so = rtp_slot<S>(T, (t & 3) + 8 * (t >> 2) + 4 * hh);
#pragma unroll
      for (int n = 0; n < 3; ++n) {
        const int col = 32 * n + j;
        if (so.valid && col < RTP_IMG) img[(int64_t)so.p * RTP_IMG + col] = acc[n][t];
      }
    }
  }
}

// ---- the radial conv's node side: the scaled node gradient (the fixed-order segmented sums are launch_seg_sum / launch_seg_mean of k_reduce.hip) ------------
// gn[n, :] = g[n, :] / max(ptr[n + 1] - ptr[n], 1): the backward of the mean, once per node, so that the indexed kernels gather plain rows
__global__ __launch_bounds__(256) void rtp_node_scale_kernel(const float* __restrict__ g, const int64_t* __restrict__ ptr, float* __restrict__ gn, int64_t N, int D) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * D) return;
  const int64_t n = idx / D, cnt = ptr[n + 1] - ptr[n];
  gn[idx] = g[idx] / (float)(cnt > 1 ? cnt : 1);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------
template <class S>      // S: a shape, or RtpIdx<shape>
static hipError_t rtp_launch(const RtpArgs& a, bool fwd, hipStream_t s) {
  const int64_t E = a.t.off[a.t.n_groups];
  const int64_t nwg = group_unit_total(a.t, RTP_EPB);
  if (nwg >= (int64_t)1 << 31) return hipErrorInvalidValue;
  const dim3 b(256);
  if (fwd) {
    if (E > 0) hipLaunchKernelGGL((rtp_edge_kernel<S, true, false, false>), dim3((unsigned)nwg), b, 0, s, a);
    return hipGetLastError();
  }
  const bool nx = a.gx || a.gsh, nh = a.gh != nullptr;
  if (E > 0 && (nx || nh)) {
    if (nx && nh) hipLaunchKernelGGL((rtp_edge_kernel<S, false, true, true>), dim3((unsigned)nwg), b, 0, s, a);
    else if (nx) hipLaunchKernelGGL((rtp_edge_kernel<S, false, true, false>), dim3((unsigned)nwg), b, 0, s, a);
    else hipLaunchKernelGGL((rtp_edge_kernel<S, false, false, true>), dim3((unsigned)nwg), b, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (a.gw2 || a.gb2) {
    const int64_t nsl = group_unit_total(a.t, a.L);
    constexpr int NCH = (RtpT<S>::NT + 3) / 4;
    if (nsl > 0) {
      hipLaunchKernelGGL((rtp_param_kernel<S>), dim3((unsigned)(nsl * NCH)), b, 0, s, a);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    return launch_slice_reduce(a.ws, a.t, a.L, ReducePart{a.gw2, a.gb2, S::W, RTP_H}, ReducePart{}, s);
  }
  return hipGetLastError();
}

int64_t rtp_backward_workspace(int32_t layer, int64_t E, int32_t n_groups) {
  if (tp_is_aa_id(layer)) {
    if (E < 0 || E >= (int64_t)1 << 31 || n_groups < 1 || n_groups > 4) return -1;
    return slice_bound(E, n_groups) * TP_LAYER_AA_W[layer - TP_AA < 3 ? layer - TP_AA : 3] * RTP_IMG * (int64_t)sizeof(float);
  }
  if (tp_is_nv4_id(layer)) {
    if (E < 0 || E >= (int64_t)1 << 31 || n_groups < 1 || n_groups > 4) return -1;
    return slice_bound(E, n_groups) * TP_LAYER_NV4_W[layer - TP_NV4 < 3 ? layer - TP_NV4 : 3] * RTP_IMG * (int64_t)sizeof(float);
  }
  if (layer < 0 || layer > 4 || E < 0 || E >= (int64_t)1 << 31 || n_groups < 1 || n_groups > 4) return -1;
  return slice_bound(E, n_groups) * TP_LAYER_W[layer < 3 ? layer : 3] * RTP_IMG * (int64_t)sizeof(float);
}

// what the forward and the backward both read: operands, group table, slice length
static RtpArgs rtp_args(const float* x_dst, const float* sh, const float* h, const int64_t* group_offsets, int n_groups, const float* w2, const float* b2) {
  RtpArgs a{};
  a.x = x_dst; a.sh = sh; a.h = h; a.w2 = w2; a.b2 = b2;
  a.t = group_table(group_offsets, n_groups);
  a.L = rtp_slice_len(group_offsets[n_groups]);
  return a;
}

hipError_t launch_rtp_forward(const ConvLayerDev& L, const float* x_dst, const float* sh, const float* h, const int64_t* group_offsets, int n_groups,
                              const float* w2, const float* b2, float* out, hipStream_t s) {
  RtpArgs a = rtp_args(x_dst, sh, h, group_offsets, n_groups, w2, b2);
  a.out = out;
  return tp_dispatch_aa(L, [&](auto shape) { return rtp_launch<decltype(shape)>(a, true, s); });
}

hipError_t launch_rtp_backward(const ConvLayerDev& L, const float* x_dst, const float* sh, const float* h, const int64_t* group_offsets, int n_groups,
                               const float* w2, const float* b2, const float* grad_out, float* grad_x, float* grad_sh, float* grad_h, float* grad_w2,
                               float* grad_b2, float* workspace, hipStream_t s) {
  RtpArgs a = rtp_args(x_dst, sh, h, group_offsets, n_groups, w2, b2);
  a.g = grad_out; a.gx = grad_x; a.gsh = grad_sh; a.gh = grad_h; a.gw2 = grad_w2; a.gb2 = grad_b2; a.ws = workspace;
  return tp_dispatch_aa(L, [&](auto shape) { return rtp_launch<decltype(shape)>(a, false, s); });
}

// ---- the radial conv ---------------------------------------------------------------------------------------------------------------------------------------------
int64_t rconv_workspace(int32_t layer, int64_t E, int32_t n_groups, int64_t n_in, int64_t n_out, int32_t backward) {
  const int64_t lim = (int64_t)1 << 31;
  const bool aa = tp_is_aa_id(layer);      // (node rows of the first family's widths)
  if (aa) layer -= TP_AA;
  const bool nv4 = !aa && tp_is_nv4_id(layer);
  if ((!nv4 && (layer < 0 || layer > 4)) || E < 0 || E >= lim || n_groups < 1 || n_groups > 4 || n_in < 0 || n_in >= lim || n_out < 0 || n_out >= lim) return -1;
  const int l = nv4 ? (layer - TP_NV4 < 3 ? layer - TP_NV4 : 3) : (layer < 3 ? layer : 3);
  int din = 0, dout = 0;
  if (nv4) { din = TP_LAYER_NV4_DIN[l]; dout = TP_LAYER_NV4_DOUT[l]; }
  else switch (l) {
    case 0: din = TpLayerShape<0>::DIN; dout = TpLayerShape<0>::DOUT; break;
    case 1: din = TpLayerShape<1>::DIN; dout = TpLayerShape<1>::DOUT; break;
    case 2: din = TpLayerShape<2>::DIN; dout = TpLayerShape<2>::DOUT; break;
    default: din = TpLayerShape<3>::DIN; dout = TpLayerShape<3>::DOUT; break;
  }
  if (!backward) return ws_pad(E * dout) * (int64_t)sizeof(float);      // the tensor product's rows
  // gn [n_out, Dout], the per-edge rows of grad_x [E, Din], the parameter images
  return (ws_pad(n_out * dout) + ws_pad(E * din)) * (int64_t)sizeof(float) + rtp_backward_workspace(aa ? TP_AA + layer : layer, E, n_groups);
}

hipError_t launch_rconv_forward(const ConvLayerDev& L, const RconvGraph& gr, const float* x_nodes, const float* sh, const float* h, const int64_t* group_offsets,
                                int n_groups, const float* w2, const float* b2, float* out_nodes, float* workspace, hipStream_t s) {
  return tp_dispatch_aa(L, [&](auto shape) {
    using S = decltype(shape);
    if (group_offsets[n_groups] == 0) return zero_async(out_nodes, gr.n_out * S::DOUT, s);
    RtpArgs a = rtp_args(x_nodes, sh, h, group_offsets, n_groups, w2, b2);
    a.xi = gr.dst;
    a.out = workspace;
    hipError_t e = rtp_launch<RtpIdx<S>>(a, true, s);
    if (e != hipSuccess) return e;
    return launch_seg_mean(workspace, gr.src_order, gr.src_ptr, out_nodes, gr.n_out, S::DOUT, s);
  });
}

hipError_t launch_rconv_backward(const ConvLayerDev& L, const RconvGraph& gr, const float* x_nodes, const float* sh, const float* h, const int64_t* group_offsets,
                                 int n_groups, const float* w2, const float* b2, const float* grad_out_nodes, float* grad_x_nodes, float* grad_sh, float* grad_h,
                                 float* grad_w2, float* grad_b2, float* workspace, hipStream_t s) {
  return tp_dispatch_aa(L, [&](auto shape) {
    using S = decltype(shape);
    const int64_t E = group_offsets[n_groups];
    if (E == 0) {
      hipError_t e = zero_async(grad_x_nodes, gr.n_in * S::DIN, s);
      if (e == hipSuccess) e = zero_async(grad_w2, (int64_t)n_groups * S::W * RTP_H, s);
      if (e == hipSuccess) e = zero_async(grad_b2, (int64_t)n_groups * S::W, s);
      return e;
    }
    float* gn = workspace;
    float* gx_rows = gn + ws_pad(gr.n_out * S::DOUT);
    float* images = gx_rows + ws_pad(E * S::DIN);
    const int64_t nb = (gr.n_out * S::DOUT + 255) / 256;
    hipLaunchKernelGGL(rtp_node_scale_kernel, dim3((unsigned)nb), dim3(256), 0, s, grad_out_nodes, gr.src_ptr, gn, gr.n_out, (int)S::DOUT);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    RtpArgs a = rtp_args(x_nodes, sh, h, group_offsets, n_groups, w2, b2);
    a.xi = gr.dst; a.gi = gr.src; a.g = gn;
    a.gx = grad_x_nodes ? gx_rows : nullptr; a.gsh = grad_sh; a.gh = grad_h; a.gw2 = grad_w2; a.gb2 = grad_b2; a.ws = images;
    e = rtp_launch<RtpIdx<S>>(a, false, s);
    if (e != hipSuccess || !grad_x_nodes) return e;
    return launch_seg_sum(gx_rows, gr.dst_order, gr.dst_ptr, grad_x_nodes, gr.n_in, S::DIN, s);
  });
}

}  // namespace ddk
