// The FasterTensorProduct shapes of the conv layers (models/tensor_layers.py:56-61), two families of four: ns = 24 / nv = 6 (the score model) and
// ns = 24 / nv = 4 (the DisCo latent encoder, models/latent_encoder.py; training ops only), and what the three files that run them share
// (k_tp.hip: the forward, k_tp_bwd.hip: its vector-Jacobian product, k_rtp.hip: the fused radial tensor product): input multiplicities A, P, Q, C of
// 0e, 1o, 1e, 0o, output multiplicities O0 .. O3, the weight blocks' row counts R0 .. R3 and their offsets B0 .. B3 in the flat weight row of W floats;
// the match of a ConvLayerDev against the shapes and the dispatch on it; the few device helpers that are the same text in more than one kernel.
// Include after ddk_internal.h.
#pragma once

#include <string.h>

namespace ddk {

// AA_: the all-atom family (below), e3nn's FullyConnectedTensorProduct with sh = 1x0e + 1x1o + 1x2e: blocks 1 and 2 end in the rows of 1o (x) 2e -> 1o and
// 1e (x) 2e -> 1e, and a block's rows lie in e3nn's instruction order in the weight row (WROW), not block after block.  Defaulted, so that the shapes of the
// two FasterTensorProduct families are the types they were
template <int A_, int P_, int Q_, int C_, int O0_, int O1_, int O2_, int O3_, bool AA_ = false>
struct TpShape {
  static constexpr int A = A_, P = P_, Q = Q_, C = C_, O0 = O0_, O1 = O1_, O2 = O2_, O3 = O3_;
  static constexpr bool AA = AA_;
  static constexpr int R0 = O0 ? A + P : 0, R1 = O1 ? A + P + Q + (AA ? P : 0) : 0, R2 = O2 ? P + Q + C + (AA ? Q : 0) : 0, R3 = O3 ? Q + C : 0;      // tensor_layers.py:56-61; all_atom_score_model.py:112-133
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
  // AA: e3nn's instructions (input irrep, sh irrep, output irrep) in its order, each a [mul_in, mul_out] matrix of the flat weight row: 0 (0e,0e,0e),
  // 1 (0e,1o,1o), 2 (1o,0e,1o), 3 (1o,1o,0e), 4 (1o,1o,1e), 5 (1o,2e,1o), 6 (1e,0e,1e), 7 (1e,1o,1o), 8 (1e,1o,0o), 9 (1e,2e,1e), 10 (0o,0e,0o), 11 (0o,1o,1e);
  // an instruction whose input or output is absent has no floats
  static constexpr int INSTR_IN(int n) { return n < 2 ? A : (n < 6 ? P : (n < 10 ? Q : C)); }
  static constexpr int INSTR_OUT(int n) {
    constexpr int o[12] = {0, 1, 1, 0, 2, 1, 2, 1, 3, 2, 3, 2};
    return O(o[n]);
  }
  static constexpr int INSTR_OFF(int n) {
    int off = 0;
    for (int i = 0; i < n; ++i) off += INSTR_IN(i) * INSTR_OUT(i);
    return off;
  }
  // where row r of block k starts in the weight row (its O(k) floats are adjacent).  The block's rows in the order of rtp_row (k_rtp.hip):
  // block 0: A rows of instruction 0, P of 3; block 1: A of 1, P of 2, Q of 7, P of 5; block 2: P of 4, Q of 6, C of 11, Q of 9; block 3: Q of 8, C of 10
  static constexpr int WROW(int k, int r) {
    if (!AA) return B(k) + r * O(k);
    if (k == 0) return r < A ? INSTR_OFF(0) + r * O0 : INSTR_OFF(3) + (r - A) * O0;
    if (k == 1) return r < A ? INSTR_OFF(1) + r * O1 : (r < A + P ? INSTR_OFF(2) + (r - A) * O1 : (r < A + P + Q ? INSTR_OFF(7) + (r - A - P) * O1 : INSTR_OFF(5) + (r - A - P - Q) * O1));
    if (k == 2) return r < P ? INSTR_OFF(4) + r * O2 : (r < P + Q ? INSTR_OFF(6) + (r - P) * O2 : (r < P + Q + C ? INSTR_OFF(11) + (r - P - Q) * O2 : INSTR_OFF(9) + (r - P - Q - C) * O2));
    return r < Q ? INSTR_OFF(8) + r * O3 : INSTR_OFF(10) + (r - Q) * O3;
  }
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

// The second family (ns = 24, nv = 4: get_irrep_seq(24, 4, False)), the same sequence with four vectors per entry.  The kernels are the same templates on
// these types: nothing in them is written for a multiplicity, only for "a vector block has at most 8 columns" (k_rtp.hip) and "an even number" (k_tp_bwd.hip).
// In the C ABI the family's layer l is the id DDK_TP_NV4 + l (include/ddk.h); no context holds such a layer, tp_family_layer below is its ConvLayerDev.
template <int I> struct TpLayerNv4;
template <> struct TpLayerNv4<0> { using type = TpShape<24, 0, 0, 0, 24, 4, 0, 0>; };
template <> struct TpLayerNv4<1> { using type = TpShape<24, 4, 0, 0, 24, 4, 4, 0>; };
template <> struct TpLayerNv4<2> { using type = TpShape<24, 4, 4, 0, 24, 4, 4, 24>; };
template <> struct TpLayerNv4<3> { using type = TpShape<24, 4, 4, 24, 24, 4, 4, 24>; };
template <int I> using TpLayerNv4Shape = typename TpLayerNv4<I>::type;
constexpr int TP_NV4 = 8;            // DDK_TP_NV4
constexpr int TP_NV4_LAYERS = 5;     // ids TP_NV4 .. TP_NV4 + 4, as layers 0..4 of the first family
constexpr int TP_LAYER_NV4_W[4] = {TpLayerNv4Shape<0>::W, TpLayerNv4Shape<1>::W, TpLayerNv4Shape<2>::W, TpLayerNv4Shape<3>::W};
constexpr int TP_LAYER_NV4_DIN[4] = {TpLayerNv4Shape<0>::DIN, TpLayerNv4Shape<1>::DIN, TpLayerNv4Shape<2>::DIN, TpLayerNv4Shape<3>::DIN};
constexpr int TP_LAYER_NV4_DOUT[4] = {TpLayerNv4Shape<0>::DOUT, TpLayerNv4Shape<1>::DOUT, TpLayerNv4Shape<2>::DOUT, TpLayerNv4Shape<3>::DOUT};
inline bool tp_is_nv4_id(int32_t layer) { return layer >= TP_NV4 && layer < TP_NV4 + TP_NV4_LAYERS; }

// The third family: the conv layers of the all-atom (confidence) model, ns = 24 / nv = 6 with sh_lmax = 2 (all_atom_score_model.py:26, 112-133): e3nn's
// FullyConnectedTensorProduct(in, 1x0e + 1x1o + 1x2e, out) on the irreps of the first family, weights in e3nn's instruction order, sh rows of 9 floats.  Only
// the radial tensor product and the radial conv (k_rtp.hip) run it; in the C ABI layer l is the id DDK_TP_AA + l, a shape that no context holds either.
template <int I> struct TpLayerAa;
template <> struct TpLayerAa<0> { using type = TpShape<24, 0, 0, 0, 24, 6, 0, 0, true>; };
template <> struct TpLayerAa<1> { using type = TpShape<24, 6, 0, 0, 24, 6, 6, 0, true>; };
template <> struct TpLayerAa<2> { using type = TpShape<24, 6, 6, 0, 24, 6, 6, 24, true>; };
template <> struct TpLayerAa<3> { using type = TpShape<24, 6, 6, 24, 24, 6, 6, 24, true>; };
template <int I> using TpLayerAaShape = typename TpLayerAa<I>::type;
constexpr int TP_AA = 16;           // DDK_TP_AA
constexpr int TP_AA_LAYERS = 5;     // ids TP_AA .. TP_AA + 4
constexpr int TP_LAYER_AA_W[4] = {TpLayerAaShape<0>::W, TpLayerAaShape<1>::W, TpLayerAaShape<2>::W, TpLayerAaShape<3>::W};
static_assert(TP_LAYER_AA_W[0] == 720 && TP_LAYER_AA_W[1] == 972 && TP_LAYER_AA_W[2] == 1224 && TP_LAYER_AA_W[3] == 1944, "e3nn's weight_numel of the four shapes");
static_assert(TpLayerAaShape<3>::INSTR_OFF(5) == 936 && TpLayerAaShape<3>::INSTR_OFF(9) == 1188 && TpLayerAaShape<3>::INSTR_OFF(11) == 1800 &&
              TpLayerAaShape<3>::WROW(1, 41) == 936 + 5 * 6 && TpLayerAaShape<3>::WROW(2, 12) == 1800, "e3nn's instruction offsets of layer 3");
inline bool tp_is_aa_id(int32_t layer) { return layer >= TP_AA && layer < TP_AA + TP_AA_LAYERS; }

// ---- host: which shape a layer has ----------------------------------------------------------------------------------------------------------------------
template <class S>
inline bool tp_shape_matches(const ConvLayerDev& L) {
  const int in[4] = {S::A, S::P, S::Q, S::C}, out[4] = {S::O0, S::O1, S::O2, S::O3};
  return memcmp(L.in_mul, in, sizeof(in)) == 0 && memcmp(L.out_mul, out, sizeof(out)) == 0;
}

inline int tp_shape_index(const ConvLayerDev& L) {      // 0..3 (nv = 6), 4..7 (nv = 4), or -1: not a FasterTensorProduct of either family
  return tp_shape_matches<TpLayerShape<0>>(L) ? 0 : (tp_shape_matches<TpLayerShape<1>>(L) ? 1 : (tp_shape_matches<TpLayerShape<2>>(L) ? 2 :
         (tp_shape_matches<TpLayerShape<3>>(L) ? 3 : (tp_shape_matches<TpLayerNv4Shape<0>>(L) ? 4 : (tp_shape_matches<TpLayerNv4Shape<1>>(L) ? 5 :
         (tp_shape_matches<TpLayerNv4Shape<2>>(L) ? 6 : (tp_shape_matches<TpLayerNv4Shape<3>>(L) ? 7 : -1)))))));
}

// the ConvLayerDev of id TP_NV4 + l: multiplicities alone (what tp_dispatch reads), no weights, the same for every context
template <class S>
inline ConvLayerDev tp_shape_only_layer() {
  ConvLayerDev L;
  const int in[4] = {S::A, S::P, S::Q, S::C}, out[4] = {S::O0, S::O1, S::O2, S::O3};
  memcpy(L.in_mul, in, sizeof(in));
  memcpy(L.out_mul, out, sizeof(out));
  L.W = S::W; L.din = S::DIN; L.dout = S::DOUT;
  L.tp_aa = S::AA;
  return L;
}
inline const ConvLayerDev& tp_family_layer(int32_t id) {      // id: tp_is_nv4_id or tp_is_aa_id
  static const ConvLayerDev table[4] = {tp_shape_only_layer<TpLayerNv4Shape<0>>(), tp_shape_only_layer<TpLayerNv4Shape<1>>(),
                                        tp_shape_only_layer<TpLayerNv4Shape<2>>(), tp_shape_only_layer<TpLayerNv4Shape<3>>()};
  static const ConvLayerDev aa[4] = {tp_shape_only_layer<TpLayerAaShape<0>>(), tp_shape_only_layer<TpLayerAaShape<1>>(),
                                     tp_shape_only_layer<TpLayerAaShape<2>>(), tp_shape_only_layer<TpLayerAaShape<3>>()};
  const int l = tp_is_aa_id(id) ? id - TP_AA : id - TP_NV4;
  return (tp_is_aa_id(id) ? aa : table)[l < 3 ? l : 3];
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
    case 4: return f(TpLayerNv4Shape<0>{});
    case 5: return f(TpLayerNv4Shape<1>{});
    case 6: return f(TpLayerNv4Shape<2>{});
    case 7: return f(TpLayerNv4Shape<3>{});
  }
  return hipErrorInvalidValue;
}

// tp_dispatch for the ops that also run the all-atom family (the radial tensor product and the radial conv): a shape-only layer with tp_aa set has the
// multiplicities of the first family's layer and the third family's type
template <class F>
inline hipError_t tp_dispatch_aa(const ConvLayerDev& L, F&& f) {
  if (!L.tp_aa) return tp_dispatch(L, f);
  switch (tp_shape_index(L)) {
    case 0: return f(TpLayerAaShape<0>{});
    case 1: return f(TpLayerAaShape<1>{});
    case 2: return f(TpLayerAaShape<2>{});
    case 3: return f(TpLayerAaShape<3>{});
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
constexpr float TP_S3_10 = 0.54772255750516611346f;      // sqrt(3/10): sqrt(dim 1o) times the amplitude 1/sqrt(10) of the Frobenius-normalised w3j(1, 2, 1)

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
