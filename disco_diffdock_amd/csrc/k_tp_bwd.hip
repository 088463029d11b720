// The vector-Jacobian product of FasterTensorProduct.forward (models/tensor_layers.py:65-116) at the reference's op boundary: from x [E, Din], sh [E, 4],
// w [E, W] and the incoming gradient g [E, Dout] to grad_x, grad_sh and grad_w, each optional.  fp32 throughout, no atomics (edges are independent), plain
// vector stores, the same bits run to run and whichever subset of the outputs is asked for (the file is compiled with -ffp-contract=off: every fused
// multiply-add below is written out, so the instantiations cannot contract the same expression differently).
//
// With the pre-weight rows of the forward (k_tp.hip; s0, v = sh)
//   U0 = [ a s0 ; (p.v)/sqrt3 ]   U1 = [ a v ; p s0 ; (q x v)/sqrt2 ]   U2 = [ (p x v)/sqrt2 ; q s0 ; c v ]   U3 = [ (q.v)/sqrt3 ; c s0 ]
// and rs_k = 1/sqrt(rows of block k):
//   grad_w block k [r, c] = rs_k U_k[r] . g_k[c]                       (needs no w)
//   G_k[r] = rs_k sum_c W_k[r, c] g_k[c]                               (a scalar for k = 0, 3, a 3-vector for k = 1, 2)
//   grad_x, grad_sh = the products of G with (s0, v) and with x        (the end of the kernel's edge loop)
//
// tp_bwd_kernel: one wave per workgroup, persistent, one edge at a time, D edges ahead in registers - the forward's stream, with a second stream going out.
//  * Lane L owns ONE input irrep: a_L (L < A), p_(L-A), q_(L-A-P) or c_(L-A-P-Q).  The rows of U that this input makes are row L of block 0e or 0o (the two
//    scalar blocks have A + P and Q + C rows: together one table TS indexed by the lane), row L of block 1o (table T1) and row L - A of block 1e (table T2):
//    the lane computes its three rows from its own input, with rs folded in, and parks them in LDS.  The same lane later owns the SAME rows of G, so the
//    products with x and sh need no exchange between lanes; only grad_sh is a sum over the wave (a fixed xor butterfly).
//  * grad_w leaves flat, 16 B per lane and 1 KB per wave instruction like the forward's read.  The (block, row, column) of each of a lane's elements is
//    decoded ONCE at kernel start into a pair of LDS byte addresses (row of TS / T1 / T2, column of g), 16 bits each in one register.  A 16-B piece of a
//    scalar block is one row times four neighbouring columns (1 ds_read_b32 + 1 ds_read_b128); a piece of a vector block is four 3-vector dot products
//    (8 ds_read_b128 from tables padded to 16 B per row and per column).  A wave instruction's 64 pieces are all of one kind except at the two block edges.
//  * The G sums read the weight row, parked flat in LDS, one block ROW per lane: scalar blocks 6 ds_read_b128 at a row stride of 24 floats, vector blocks
//    3 ds_read_b64 at a stride of 6 floats (nv = 4: 2 at a stride of 4).  Bank mapping: 6-float rows read 8 B per lane are conflict-free (banks 6 r mod 64, all
//    even and distinct over 32 rows; 4-float rows repeat after 16 rows: rows r and r + 16 meet, not measured apart).  24-float rows start on banks 24 r mod 64 = 8 (3 r mod 8): eight starts, and rows r, r + 8 of a ds_read_b128 lane group would meet.  The
//    lane groups of ds_read_b128 take lanes of two neighbouring octets from each half of a 32-lane window ({0-3, 12-15, 20-27}, ...), so reading the six
//    16-B pieces of a row in the order j ^ 1 in lanes 16-31 and 48-63 moves those lanes to the odd 4-bank slots; the column operand g follows the same order.
#include <stdlib.h>

#include "ddk_internal.h"
#include "k_tp_shape.h"

namespace ddk {

struct TpBArgs {
  const float* x; const float* sh; const float* w; const float* g;
  float* gx; float* gsh; float* gw;
  int64_t E;
};

// the LDS image of one workgroup, byte offsets: the flat weight row, TS [64] floats, T1 / T2 [64] float4, g flat [128] floats, g's vector columns [16] float4
template <class S, bool NX>
struct TpbLds {
  static constexpr int W_OFF = 0, TS_OFF = NX ? S::NV * 64 * 16 : 0, T1_OFF = TS_OFF + 256, T2_OFF = T1_OFF + 1024, GF_OFF = T2_OFF + 1024,
                       GT_OFF = GF_OFF + 512, BYTES = GT_OFF + 256;
  static_assert(BYTES < 65536, "the decode keeps LDS byte addresses in 16 bits");
};
template <class S, bool NX> struct TpbRow { float4 w[NX ? S::NV : 1]; float xi[3]; float4 sh; float g0, g1; float gc[3]; };

// what a lane is: its input irrep (role 0..3 = a, p, q, c; 4 = none) and where that input sits in the node row
template <class S>
struct TpbLane {
  int role, xoff, xstep;
  __device__ __forceinline__ explicit TpbLane(int lane) {
    role = lane < S::A ? 0 : (lane < S::A + S::P ? 1 : (lane < S::A + S::P + S::Q ? 2 : (lane < S::A + S::P + S::Q + S::C ? 3 : 4)));
    xoff = role == 0 ? lane : (role == 1 || role == 2 ? S::A + 3 * (lane - S::A) : (role == 3 ? S::XC + (lane - S::A - S::P - S::Q) : 0));
    xstep = role == 1 || role == 2 ? 1 : 0;
  }
};

template <class S, bool NW, bool NX>
__device__ __forceinline__ void tpb_request(const TpBArgs& a, int64_t e, int lane, const TpbLane<S>& ln, TpbRow<S, NX>& R) {
  if (NX) tp_read_row<S>(a.w + e * S::W, lane, R.w);
  const float* xr = a.x + e * S::DIN;
#pragma unroll
  for (int k = 0; k < 3; ++k) R.xi[k] = ln.role < 4 ? xr[ln.xoff + k * ln.xstep] : 0.f;      // a scalar input three times over
  const tp_f4 q = *reinterpret_cast<const tp_f4*>(a.sh + e * 4);
  R.sh = make_float4(q.x, q.y, q.z, q.w);
  const float* gr = a.g + e * S::DOUT;
  R.g0 = lane < S::DOUT ? gr[lane] : 0.f;
  R.g1 = lane + 64 < S::DOUT ? gr[lane + 64] : 0.f;
  if (NW) {
#pragma unroll
    for (int k = 0; k < 3; ++k) R.gc[k] = lane < S::O1 + S::O2 ? gr[S::O0 + 3 * lane + k] : 0.f;      // vector column `lane` of g
  }
}

template <class S, int D, bool NW, bool NX>
__global__ __launch_bounds__(64) void tp_bwd_kernel(TpBArgs a) {
  using M = TpbLds<S, NX>;
  static_assert(S::O0 > 0 && S::O0 % 4 == 0 && (S::O3 == 0 || S::O3 == S::O0) && S::B1 % 4 == 0 && S::B2 % 4 == 0 && S::B3 % 4 == 0, "a 16-B piece of a scalar block is one row");
  static_assert(S::O3 == 0 || (S::O0 + 3 * S::O1 + 3 * S::O2) % 4 == 0, "g of block 0o is read 16 B at a time");
  static_assert(S::O1 % 2 == 0 && S::O2 % 2 == 0 && S::O1 + S::O2 <= 16, "vector rows are read as 8-B pairs (nv = 6: three, nv = 4: two)");
  static_assert(S::A + S::P + S::Q + S::C <= 64 && S::R0 + S::R3 <= 64 && S::R1 <= 64 && S::A + S::R2 <= 64 && S::DOUT <= 128, "one lane per input irrep and per block row");
  static_assert(S::R0 == S::A + S::P, "block 0o's rows follow block 0e's in the lane order");
  __shared__ float4 smem4[M::BYTES / 16];
  char* sm = reinterpret_cast<char*>(smem4);
  const int lane = threadIdx.x;
  const int64_t stride = gridDim.x;
  int64_t e = blockIdx.x;
  const TpbLane<S> ln(lane);
  const int role = ln.role;
  const float inv_s3 = TP_INV_S3, inv_s2 = TP_INV_S2;
  const float rs0 = TP_RS(S::R0), rs1 = TP_RS(S::R1), rs2 = TP_RS(S::R2), rs3 = TP_RS(S::R3);
  const float rss = lane < S::R0 ? rs0 : rs3;      // the lane's row of TS belongs to block 0e or 0o

  // grad_w: (row address) | (column address) << 16 of the lane's 4 NV elements, and which of its 16-B pieces lie in a vector block
  int dec[NW ? S::NV : 1][4];
  unsigned vecmask = 0;
  if (NW) {
#pragma unroll
    for (int t = 0; t < S::NV; ++t) {
      const int f = 64 * t + lane;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int idx = f < S::W / 4 ? 4 * f + j : 0;
        const int blk = idx < S::B1 ? 0 : (idx < S::B2 ? 1 : (idx < S::B3 ? 2 : 3));
        int r = 0, c = 0, ua = 0, ga = 0;
        if (blk == 0) { r = idx / S::O0; c = idx - r * S::O0; ua = M::TS_OFF + 4 * r; ga = M::GF_OFF + 4 * c; }
        if (blk == 1 && S::O1 > 0) { const int i = idx - S::B1; r = i / (S::O1 > 0 ? S::O1 : 1); c = i - r * S::O1; ua = M::T1_OFF + 16 * r; ga = M::GT_OFF + 16 * c; }
        if (blk == 2 && S::O2 > 0) { const int i = idx - S::B2; r = i / (S::O2 > 0 ? S::O2 : 1); c = i - r * S::O2; ua = M::T2_OFF + 16 * (r + S::A); ga = M::GT_OFF + 16 * (S::O1 + c); }
        if (blk == 3 && S::O3 > 0) { const int i = idx - S::B3; r = i / (S::O3 > 0 ? S::O3 : 1); c = i - r * S::O3; ua = M::TS_OFF + 4 * (S::R0 + r); ga = M::GF_OFF + 4 * (S::O0 + 3 * S::O1 + 3 * S::O2 + c); }
        dec[t][j] = ua | (ga << 16);
        if (j == 0 && (blk == 1 || blk == 2)) vecmask |= 1u << t;
      }
    }
  }
  // G: the lane's rows of the parked weight row.  Scalar blocks: row `lane` of 0e, then the rows of 0o; block 1o: row `lane`; block 1e: row `lane - A`
  const bool onS = lane < S::R0 + S::R3, on1 = lane < S::R1, on2 = lane >= S::A && lane < S::A + S::R2;
  const int wS = onS ? 4 * (lane < S::R0 ? S::B0 + lane * S::O0 : S::B3 + (lane - S::R0) * S::O3) : 0;
  const int gS = M::GF_OFF + (lane < S::R0 || S::O3 == 0 ? 0 : 4 * (S::O0 + 3 * S::O1 + 3 * S::O2));      // (16-B aligned: an idle lane too reads 16 B)
  const int rot = ((lane >> 4) & 1) << 4;      // the order of a 24-float row's six pieces: see the bank mapping above
  const int w1 = on1 ? 4 * (S::B1 + lane * S::O1) : 0, w2 = on2 ? 4 * (S::B2 + (lane - S::A) * S::O2) : 0;

  TpbRow<S, NX> R[D];
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (e + d * stride < a.E) tpb_request<S, NW, NX>(a, e + d * stride, lane, ln, R[d]);
  for (;;) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (e >= a.E) return;
      if (NX) {
#pragma unroll
        for (int t = 0; t < S::NV; ++t) smem4[64 * t + lane] = R[d].w[t];
      }
      const float i0 = R[d].xi[0], i1 = R[d].xi[1], i2 = R[d].xi[2];
      const float s0 = R[d].sh.x, vx = R[d].sh.y, vy = R[d].sh.z, vz = R[d].sh.w;
      const float g0 = R[d].g0, g1 = R[d].g1;
      float* gf = reinterpret_cast<float*>(sm + M::GF_OFF);
      gf[lane] = g0;
      gf[64 + lane] = g1;
      if (NW) {
        if (lane < 16) *reinterpret_cast<float4*>(sm + M::GT_OFF + 16 * lane) = make_float4(R[d].gc[0], R[d].gc[1], R[d].gc[2], 0.f);
      }
      if (e + (int64_t)D * stride < a.E) tpb_request<S, NW, NX>(a, e + (int64_t)D * stride, lane, ln, R[d]);
      if (NW) {
        // the lane's rows of U, rs folded in: scalar (x) s0, scalar (x) v, vector s0, (vector x v)/sqrt2, (vector . v)/sqrt3
        const float dot = fmaf(i2, vz, fmaf(i1, vy, i0 * vx)) * inv_s3;
        const float cx = fmaf(i1, vz, -(i2 * vy)) * inv_s2, cy = fmaf(i2, vx, -(i0 * vz)) * inv_s2, cz = fmaf(i0, vy, -(i1 * vx)) * inv_s2;
        const float us = role == 0 || role == 3 ? i0 * s0 : (role < 4 ? dot : 0.f);
        float u1x = 0.f, u1y = 0.f, u1z = 0.f, u2x = 0.f, u2y = 0.f, u2z = 0.f;
        if (role == 0) { u1x = i0 * vx; u1y = i0 * vy; u1z = i0 * vz; }
        if (role == 1) { u1x = i0 * s0; u1y = i1 * s0; u1z = i2 * s0; u2x = cx; u2y = cy; u2z = cz; }
        if (role == 2) { u1x = cx; u1y = cy; u1z = cz; u2x = i0 * s0; u2y = i1 * s0; u2z = i2 * s0; }
        if (role == 3) { u2x = i0 * vx; u2y = i0 * vy; u2z = i0 * vz; }
        reinterpret_cast<float*>(sm + M::TS_OFF)[lane] = us * rss;
        *reinterpret_cast<float4*>(sm + M::T1_OFF + 16 * lane) = make_float4(u1x * rs1, u1y * rs1, u1z * rs1, 0.f);
        *reinterpret_cast<float4*>(sm + M::T2_OFF + 16 * lane) = make_float4(u2x * rs2, u2y * rs2, u2z * rs2, 0.f);
      }
      __syncthreads();
      if (NW) {
        float* gwr = a.gw + e * S::W;
#pragma unroll
        for (int t = 0; t < S::NV; ++t) {
          const int f = 64 * t + lane;
          if ((t + 1) * 64 <= S::W / 4 || f < S::W / 4) {
            tp_f4 o;
            if ((vecmask >> t) & 1u) {
              float ov[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const float4 u = *reinterpret_cast<const float4*>(sm + (dec[t][j] & 0xffff));
                const float4 gc = *reinterpret_cast<const float4*>(sm + ((unsigned)dec[t][j] >> 16));
                ov[j] = fmaf(u.z, gc.z, fmaf(u.y, gc.y, u.x * gc.x));
              }
              o.x = ov[0]; o.y = ov[1]; o.z = ov[2]; o.w = ov[3];
            } else {
              const float u = *reinterpret_cast<const float*>(sm + (dec[t][0] & 0xffff));
              const float4 gc = *reinterpret_cast<const float4*>(sm + ((unsigned)dec[t][0] >> 16));
              o.x = u * gc.x; o.y = u * gc.y; o.z = u * gc.z; o.w = u * gc.w;
            }
            *reinterpret_cast<tp_f4*>(gwr + 4 * f) = o;
          }
        }
      }
      if (NX) {
        // G of the lane's rows
        float Gs = 0.f, G1x = 0.f, G1y = 0.f, G1z = 0.f, G2x = 0.f, G2y = 0.f, G2z = 0.f;
        {
          float acc = 0.f;
#pragma unroll
          for (int j = 0; j < S::O0 / 4; ++j) {
            const int o = (16 * j) ^ rot;
            const float4 wv = *reinterpret_cast<const float4*>(sm + wS + o);
            const float4 gv = *reinterpret_cast<const float4*>(sm + gS + o);
            acc = fmaf(wv.x, gv.x, acc); acc = fmaf(wv.y, gv.y, acc); acc = fmaf(wv.z, gv.z, acc); acc = fmaf(wv.w, gv.w, acc);
          }
          Gs = onS ? acc * rss : 0.f;
        }
        if (S::O1 > 0) {
          float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
          for (int c2 = 0; c2 < S::O1 / 2; ++c2) {
            const float2 wv = *reinterpret_cast<const float2*>(sm + w1 + 8 * c2);
            const int k0 = S::O0 + 6 * c2;
            ax = fmaf(wv.x, tp_row_val(g0, g1, k0), ax); ay = fmaf(wv.x, tp_row_val(g0, g1, k0 + 1), ay); az = fmaf(wv.x, tp_row_val(g0, g1, k0 + 2), az);
            ax = fmaf(wv.y, tp_row_val(g0, g1, k0 + 3), ax); ay = fmaf(wv.y, tp_row_val(g0, g1, k0 + 4), ay); az = fmaf(wv.y, tp_row_val(g0, g1, k0 + 5), az);
          }
          if (on1) { G1x = ax * rs1; G1y = ay * rs1; G1z = az * rs1; }
        }
        if (S::O2 > 0) {
          float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
          for (int c2 = 0; c2 < S::O2 / 2; ++c2) {
            const float2 wv = *reinterpret_cast<const float2*>(sm + w2 + 8 * c2);
            const int k0 = S::O0 + 3 * S::O1 + 6 * c2;
            ax = fmaf(wv.x, tp_row_val(g0, g1, k0), ax); ay = fmaf(wv.x, tp_row_val(g0, g1, k0 + 1), ay); az = fmaf(wv.x, tp_row_val(g0, g1, k0 + 2), az);
            ax = fmaf(wv.y, tp_row_val(g0, g1, k0 + 3), ax); ay = fmaf(wv.y, tp_row_val(g0, g1, k0 + 4), ay); az = fmaf(wv.y, tp_row_val(g0, g1, k0 + 5), az);
          }
          if (on2) { G2x = ax * rs2; G2y = ay * rs2; G2z = az * rs2; }
        }
        // the lane's input against its rows of G (role a: G0, G1; p: G0, G1, G2; q: G3, G1, G2; c: G3, G2)
        if (a.gx) {
          float* o = a.gx + e * S::DIN + ln.xoff;
          if (role == 0) {             // s0 G0 + v . G1
            o[0] = fmaf(s0, Gs, fmaf(vz, G1z, fmaf(vy, G1y, vx * G1x)));
          } else if (role == 1) {      // v G0/sqrt3 + s0 G1 + (v x G2)/sqrt2
            const float k3 = Gs * inv_s3;
            o[0] = fmaf(vx, k3, fmaf(s0, G1x, fmaf(vy, G2z, -(vz * G2y)) * inv_s2));
            o[1] = fmaf(vy, k3, fmaf(s0, G1y, fmaf(vz, G2x, -(vx * G2z)) * inv_s2));
            o[2] = fmaf(vz, k3, fmaf(s0, G1z, fmaf(vx, G2y, -(vy * G2x)) * inv_s2));
          } else if (role == 2) {      // (v x G1)/sqrt2 + s0 G2 + v G3/sqrt3
            const float k3 = Gs * inv_s3;
            o[0] = fmaf(vx, k3, fmaf(s0, G2x, fmaf(vy, G1z, -(vz * G1y)) * inv_s2));
            o[1] = fmaf(vy, k3, fmaf(s0, G2y, fmaf(vz, G1x, -(vx * G1z)) * inv_s2));
            o[2] = fmaf(vz, k3, fmaf(s0, G2z, fmaf(vx, G1y, -(vy * G1x)) * inv_s2));
          } else if (role == 3) {      // v . G2 + s0 G3
            o[0] = fmaf(s0, Gs, fmaf(vz, G2z, fmaf(vy, G2y, vx * G2x)));
          }
        }
        if (a.gsh) {
          // grad_s0 = sum a G0 + p . G1 + q . G2 + c G3;  grad_v = sum a G1 + p G0/sqrt3 + (G2 x p)/sqrt2 + (G1 x q)/sqrt2 + q G3/sqrt3 + c G2
          float ts = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
          if (role == 0) { ts = i0 * Gs; tx = i0 * G1x; ty = i0 * G1y; tz = i0 * G1z; }
          if (role == 3) { ts = i0 * Gs; tx = i0 * G2x; ty = i0 * G2y; tz = i0 * G2z; }
          if (role == 1 || role == 2) {
            const float Ax = role == 1 ? G1x : G2x, Ay = role == 1 ? G1y : G2y, Az = role == 1 ? G1z : G2z;      // the block that takes the input times s0
            const float Bx = role == 1 ? G2x : G1x, By = role == 1 ? G2y : G1y, Bz = role == 1 ? G2z : G1z;      // the block that takes it crossed with v
            const float k3 = Gs * inv_s3;
            ts = fmaf(i2, Az, fmaf(i1, Ay, i0 * Ax));
            tx = fmaf(i0, k3, fmaf(By, i2, -(Bz * i1)) * inv_s2);
            ty = fmaf(i1, k3, fmaf(Bz, i0, -(Bx * i2)) * inv_s2);
            tz = fmaf(i2, k3, fmaf(Bx, i1, -(By * i0)) * inv_s2);
          }
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) {
            ts += __shfl_xor(ts, m); tx += __shfl_xor(tx, m); ty += __shfl_xor(ty, m); tz += __shfl_xor(tz, m);
          }
          if (lane == 0) {
            tp_f4 o;
            o.x = ts; o.y = tx; o.z = ty; o.w = tz;
            *reinterpret_cast<tp_f4*>(a.gsh + e * 4) = o;
          }
        }
      }
      e += stride;
      __syncthreads();
    }
  }
}

hipError_t launch_tp_backward(const ConvLayerDev& L, const float* x_dst, const float* sh, const float* w, const float* grad_out, int64_t E,
                              float* grad_x, float* grad_sh, float* grad_w, hipStream_t s) {
  if (E == 0) return hipSuccess;
  const TpBArgs a{x_dst, sh, w, grad_out, grad_x, grad_sh, grad_w, E};
  const bool nw = grad_w != nullptr, nx = grad_x != nullptr || grad_sh != nullptr;
  if (!nw && !nx) return hipErrorInvalidValue;
  return tp_dispatch(L, [&](auto shape) {
    using S = decltype(shape);
    const dim3 g = tp_persistent_grid(E), b(64);      // as many waves as the forward's
    if (nw && nx) hipLaunchKernelGGL((tp_bwd_kernel<S, 2, true, true>), g, b, 0, s, a);
    else if (nw) hipLaunchKernelGGL((tp_bwd_kernel<S, 2, true, false>), g, b, 0, s, a);
    else hipLaunchKernelGGL((tp_bwd_kernel<S, 2, false, true>), g, b, 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace ddk
