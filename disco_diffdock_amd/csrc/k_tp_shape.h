// The four FasterTensorProduct shapes of the score model's conv layers (models/tensor_layers.py:56-61) and what the three files that run them share
// (k_tp.hip: the forward, k_tp_bwd.hip: its vector-Jacobian product, k_rtp.hip: the fused radial tensor product): input multiplicities A, P, Q, C of
// 0e, 1o, 1e, 0o, output multiplicities O0 .. O3, the weight blocks' row counts R0 .. R3 and their offsets B0 .. B3 in the flat weight row of W floats;
// the match of a ConvLayerDev against the shapes and the dispatch on it; the few device helpers that are the same text in more than one kernel.
// Include after ddk_internal.h.
#pragma once

#include <string.h>

namespace ddk {

template <int A_, int P_, int Q_, int C_, int O0_, int O1_, int O2_, int O3_>
struct TpShape {
  static constexpr int A = A_, P = P_, Q = Q_, C = C_, O0 = O0_, O1 = O1_, O2 = O2_, O3 = O3_;
  static constexpr int R0 = O0 ? A + P : 0, R1 = O1 ? A + P + Q : 0, R2 = O2 ? P + Q + C : 0, R3 = O3 ? Q + C : 0;      // tensor_layers.py:56-61
  static constexpr int B0 = 0, B1 = B0 + R0 * O0, B2 = B1 + R1 * O1, B3 = B2 + R2 * O2, W = B3 + R3 * O3;
  static constexpr int DIN = A + 3 * P + 3 * Q + C, DOUT = O0 + 3 * O1 + 3 * O2 + O3;
  static constexpr int NV = (W / 4 + 63) / 64;       // 16-B loads per lane and row
  static constexpr int XC = A + 3 * P + 3 * Q;       // first 0o input
  // Block k by index: rows, columns, offset in the weight row, offset in an out row, 3-vector columns.  For a k known at COMPILE time (a template
  // argument, a constexpr, an array bound).  Where a kernel selects by a lane's or a tile's block at run time its ?: chain stays written out unless
  // the kernel's assembly is the same either way (rtp_param_kernel's OUT_OFF and vec are): through these the compiler may turn the selects into
  // exec-masked branches and allocate registers differently, and the instruction streams are what was measured.
  static constexpr int R(int k) { return k == 0 ? R0 : (k == 1 ? R1 : (k == 2 ? R2 : R3)); }
  static constexpr int O(int k) { return k == 0 ? O0 : (k == 1 ? O1 : (k == 2 ? O2 : O3)); }
  static constexpr int B(int k) { return k == 0 ? B0 : (k == 1 ? B1 : (k == 2 ? B2 : B3)); }
  static constexpr int OUT_OFF(int k) { return k == 0 ? 0 : (k == 1 ? O0 : (k == 2 ? O0 + 3 * O1 : O0 + 3 * O1 + 3 * O2)); }
  static constexpr bool vec(int k) { return k == 1 || k == 2; }
  static_assert(A % 8 == 0 && C % 8 == 0 && (A == C || A == 0 || C == 0) && (C == 0 || XC % 4 == 0), "phase A is walked in two halves");
  static_assert(W % 4 == 0 && DIN <= 128 && O0 + O1 + O2 + O3 <= 64 && P <= 8 && Q <= 8, "shape outside the kernel's layout");
};

// The shapes (ns = 24, nv = 6; get_irrep_seq, tensor_layers.py:12-27): conv layer l takes entry min(l, 3) of 24x0e [+ 6x1o [+ 6x1e [+ 24x0o]]] to
// entry min(l + 1, 3), so layer l has shape min(l, 3): layers 3 and later share shape 3.
template <int I> struct TpLayer;
template <> struct TpLayer<0> { using type = TpShape<24, 0, 0, 0, 24, 6, 0, 0>; };
template <> struct TpLayer<1> { using type = TpShape<24, 6, 0, 0, 24, 6, 6, 0>; };
template <> struct TpLayer<2> { using type = TpShape<24, 6, 6, 0, 24, 6, 6, 24>; };
template <> struct TpLayer<3> { using type = TpShape<24, 6, 6, 24, 24, 6, 6, 24>; };
template <int I> using TpLayerShape = typename TpLayer<I>::type;
constexpr int TP_LAYER_W[4] = {TpLayerShape<0>::W, TpLayerShape<1>::W, TpLayerShape<2>::W, TpLayerShape<3>::W};

// ---- host: which shape a layer has ----------------------------------------------------------------------------------------------------------------------
template <class S>
inline bool tp_shape_matches(const ConvLayerDev& L) {
  const int in[4] = {S::A, S::P, S::Q, S::C}, out[4] = {S::O0, S::O1, S::O2, S::O3};
  return memcmp(L.in_mul, in, sizeof(in)) == 0 && memcmp(L.out_mul, out, sizeof(out)) == 0;
}

inline int tp_shape_index(const ConvLayerDev& L) {      // 0..3, or -1: not a FasterTensorProduct of this model family (ddk_create refuses other ns / nv)
  return tp_shape_matches<TpLayerShape<0>>(L) ? 0 : (tp_shape_matches<TpLayerShape<1>>(L) ? 1 : (tp_shape_matches<TpLayerShape<2>>(L) ? 2 :
         (tp_shape_matches<TpLayerShape<3>>(L) ? 3 : -1)));
}

// f(S{}) with the layer's shape type S, e.g. [&](auto shape) { using S = decltype(shape); ... }; hipErrorInvalidValue for a layer without one (the C
// entry points ask tp_shape_index first, so they never see that value from here)
template <class F>
inline hipError_t tp_dispatch(const ConvLayerDev& L, F&& f) {
  switch (tp_shape_index(L)) {
    case 0: return f(TpLayerShape<0>{});
    case 1: return f(TpLayerShape<1>{});
    case 2: return f(TpLayerShape<2>{});
    case 3: return f(TpLayerShape<3>{});
  }
  return hipErrorInvalidValue;
}

// the grid of the two persistent one-wave-per-workgroup kernels (tp_col_kernel, tp_bwd_kernel): 16 waves per CU cover the occupancy of every
// instantiation (3 .. 5 waves per SIMD), each with one edge in hand and two in flight
inline dim3 tp_persistent_grid(int64_t E) {
  const int64_t cap = 256 * 16;
  return dim3((unsigned)(E < cap ? E : cap));
}

// ---- device -------------------------------------------------------------------------------------------------------------------------------------------------
typedef float tp_f4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr float TP_INV_S3 = 0.57735026918962576451f, TP_INV_S2 = 0.70710678118654752440f;      // 1/sqrt(3), 1/sqrt(2)

// the scale 1/sqrt(R_k) of a weight block of `rows` rows (tensor_layers.py:89-92); an absent block: 1.  A macro: as an inline function the same
// expression gives three kernels another instruction stream
#define TP_RS(rows) (1.0f / sqrtf((float)((rows) > 0 ? (rows) : 1)))

__device__ __forceinline__ float tp_rl(float v, int k) {      // v_readlane_b32 on the bit pattern (the builtin is typed int: a plain call would convert the VALUE)
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), k));
}

// element k of a row of up to 128 floats that the wave holds in two registers (lane L: elements L and 64 + L), as a wave-uniform value (k is a
// compile-time constant)
__device__ __forceinline__ float tp_row_val(float r0, float r1, int k) {
  return tp_rl(k < 64 ? r0 : r1, k < 64 ? k : k - 64);
}

// the weight row of an edge, W floats at `row`, read flat: 16 B per lane and 1 KB per wave instruction, piece 64 t + lane into w[t] (pieces past the
// row's end are not read and w[t] keeps its value).  Default cache policy: non-temporal loads measured 1-3 % slower on this stream
template <class S>
__device__ __forceinline__ void tp_read_row(const float* row, int lane, float4* w) {
  const float4* wr = reinterpret_cast<const float4*>(row);
#pragma unroll
  for (int t = 0; t < S::NV; ++t) {
    const int f = 64 * t + lane;
    if ((t + 1) * 64 <= S::W / 4 || f < S::W / 4) {
      const tp_f4 q = *reinterpret_cast<const tp_f4*>(wr + f);
      w[t] = make_float4(q.x, q.y, q.z, q.w);
    }
  }
}

}  // namespace ddk
